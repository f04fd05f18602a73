"""Fixed-seed inputs of the exact-fp32 attention bit-identity cases, shared by tests/golden/make_golden_attention_bits.py
(which records the hashes) and tests/test_hip_attention_fp32_bits.py (which asserts them).

The shapes are the smallest at which each part of attn_fwd_pipe's tile loop can go wrong: one tile alone (prologue, the peeled
last tile, ragged tail), two tiles, odd and even tile counts against the two-tile unrolling, 4- and 8-wave blocks (the entry
picks 8 waves above 128 rows), head dim 32 in both block widths, masked keys with a wholly dead tile, and the rare fix-up path.
"""
import hashlib

import torch

#        name               B  H  T    dh  mask kind
DIRECT = [("t31",           1, 2, 31,  64, None),
          ("t64",           1, 2, 64,  64, None),
          ("t65",           1, 2, 65,  64, None),
          ("t128",          1, 2, 128, 64, None),
          ("t129",          1, 4, 129, 64, None),
          ("t192",          2, 4, 192, 64, None),
          ("t256",          1, 4, 256, 64, None),
          ("t320",          1, 4, 320, 64, None),
          ("dh32_t65",      1, 8, 65,  32, None),
          ("dh32_t300",     1, 8, 300, 32, None),
          ("mask_t200",     2, 4, 200, 64, "random"),
          ("mask_dh32_t65", 1, 8, 65,  32, "random"),
          ("mask_dead70",   1, 4, 256, 64, "dead70"),      # keys 186..255 masked: tile 3 (keys 192..255) is wholly dead
          # the inputs of test_hip_attention_maps.py::test_probs_kernel_against_float64 (larger logits: the fix-up runs in
          # many blocks, with the masked kernels' key-bias adds right behind each block's first MFMA), 4- and 8-wave blocks
          ("mask_dh32_t97_g3",  2, 2, 97,  32, "holes_pad"),
          ("mask_dh32_t320_g3", 2, 2, 320, 32, "holes_pad")]
SPIKED = ["spike_late", "spike_twice"]
PACKED_LENGTHS = [37, 64, 65, 129, 300]
PACKED_MODEL = dict(H=4, d=256, L=2, wseed=23)            # head dim 64
LIMIT_RANDOM = 2e-5            # tests/test_hip_parity.py: test_attention_kernel
LIMIT_RESCALE = 5e-5           # tests/test_hip_parity.py: test_attention_online_softmax_rescale_branch


def direct_inputs(synth, name):
    """(q, k, v, mask or None, scale) of a DIRECT case: test_attention_kernel's recipe."""
    _, B, H, T, dh, kind = next(c for c in DIRECT if c[0] == name)
    g = torch.Generator().manual_seed(1000 * dh + T + (7 if kind else 0))
    q, k, v = (torch.randn(B, H, T, dh, generator=g) * 2.0 for _ in range(3))
    mask = None
    if kind == "holes_pad":                                # video 1 is padded from two thirds on, video 0 has a few holes
        q, k, v = q * 1.5, k * 1.5, v * 0.5
        mask = torch.zeros(B, T, dtype=torch.bool)
        mask[1, (2 * T) // 3:] = True
        mask[0, 1::5] = True
        return q, k, v, mask, 256.0 ** -0.5
    if kind == "random":
        mask = synth.random_mask(B, T, 3)
    elif kind == "dead70":
        mask = torch.zeros(B, T, dtype=torch.bool)
        mask[:, T - 70:] = True
    return q, k, v, mask, (H * dh) ** -0.5


def spiked_inputs(name):
    """The construction of test_attention_online_softmax_rescale_branch (T = 512, scale 1): key 300 spikes against every
    query, so the running maximum jumps by far more than 2^8 in tile 4's second 32-key block (keys 288..319) - the fix-up
    rewrites the bias, and the block already in flight (keys 320..351) was started with the stale one.  spike_twice adds a
    half-height spike at key 270, in the first block of the same tile: two raises in consecutive blocks."""
    B, H, T, dh = 1, 4, 512, 64
    g = torch.Generator().manual_seed(99)
    q, k, v = (torch.randn(B, H, T, dh, generator=g) for _ in range(3))
    k[:, :, 300] = q.mean(dim=2) * 50.0 + 20.0
    k[:, :, 77] = -k[:, :, 300]
    if name == "spike_twice":
        k[:, :, 270] = 0.5 * k[:, :, 300]
    return q, k, v, None, 1.0


def attn_ref(q, k, v, mask, scale):
    """float64 reference: the arithmetic of tests/test_hip_parity.py's _attn_ref."""
    s = torch.matmul(q.double(), k.double().transpose(2, 3)) * scale
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=3), v.double())
    B, H, T, dh = q.shape
    return o.permute(0, 2, 1, 3).reshape(B, T, H * dh)


def run_direct(pkg, q, k, v, mask, scale, dev):
    """vs_attention_f32 on the device; returns the [B, T, H*dh] output on the host."""
    lib = pkg._lib.load()
    B, H, T, dh = q.shape
    dq, dk, dv = q.to(dev), k.to(dev), v.to(dev)
    dm = mask.to(dev) if mask is not None else None
    out = torch.full((B, T, H * dh), float("nan"), device=dev)
    pkg._lib.check(lib.vs_attention_f32(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dm.data_ptr() if dm is not None else None,
                                        out.data_ptr(), B, H, T, dh, scale, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu()


def packed_model(pkg, dev):
    c = PACKED_MODEL
    m = pkg.SimNet(num_heads=c["H"], d_model=c["d"], num_layers=c["L"], sparsity=0.0, dropout=0.3)
    m.load_state_dict(pkg.synth.make_state_dict(c["d"], c["L"], c["wseed"]), strict=True)
    return m.to(dev).eval()


def packed_videos(synth):
    return [synth.make_features(1, t, 300 + i, "pool5")[0] for i, t in enumerate(PACKED_LENGTHS)]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
