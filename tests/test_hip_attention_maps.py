"""GPU: the attention maps on request (include/vs_inspect.h, SimNet.attention_maps / attention_summary) against the float64
fixtures made by the imported reference (tests/golden/make_golden_attn.py), against float64 numpy at the kernel level, and
their contract: bit-equal logits, determinism, batch independence, layer selection, mode independence, no [T,T] allocation.

Tolerance: tolerances.FP32_TOL (1e-4 absolute) on every map entry of a valid query row, on `received` and on the entropy
(nats) of valid rows.  The reference's own fp32 path is within 2.9e-5 of its float64 run on all three for gains <= 8
(each fixture records its own figure as `ref32`).  Every test prints what it measured before it asserts."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_cases
from conftest import GOLDEN
from tolerances import FP32_TOL

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _model(vsa, c, sd, **kw):
    m = vsa.SimNet(num_heads=c["H"], d_model=c["d"], num_layers=c["L"], sparsity=0.0, dropout=0.3,
                   use_cls=bool(c.get("use_cls")), **kw)
    m.load_state_dict(sd, strict=True)
    return m.to(_dev()).eval()


def _case(name):
    return next(c for c in attn_cases.CASES if c["name"] == name)


def _inputs(vsa, c):
    sd, x, mask = attn_cases.build(vsa.synth, c)
    return sd, x.to(_dev()), (None if mask is None else mask.to(_dev())), mask


def _key_dead(c, mask):
    """bool [B, N]: masked key columns (the class token is never masked)"""
    return ~attn_cases.valid_rows(c, mask)


# ---- 1. golden parity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", attn_cases.CASES, ids=lambda c: c["name"])
def test_maps_and_summary_match_the_float64_goldens(vsa, case):
    z = np.load(os.path.join(GOLDEN, case["name"] + ".npz"))
    assert json.loads(str(z["cfg"])) == case
    sd, x, m, mask = _inputs(vsa, case)
    model = _model(vsa, case, sd)
    valid = attn_cases.valid_rows(case, mask)
    dead = _key_dead(case, mask)
    logits, received, entropy = model.attention_summary(x, m)
    torch.cuda.synchronize()
    L, B, H = case["L"], case["B"], case["H"]
    N = case["T"] + (1 if case.get("use_cls") else 0)
    assert received.shape == entropy.shape == (L, B, H, N) and logits.shape == (B, N, 1)
    rec, ent = received.cpu().numpy().astype(np.float64), entropy.cpu().numpy().astype(np.float64)
    vq = np.broadcast_to(valid[None, :, None, :], ent.shape)
    d_rec = np.abs(rec - z["received"]).max()
    d_ent = np.abs(ent - z["entropy"])[vq].max()
    print("%s: received %.2e entropy %.2e (reference fp32: %s)" % (case["name"], d_rec, d_ent, z["ref32"].max(axis=0)))
    assert np.all(rec[np.broadcast_to(dead[None, :, None, :], rec.shape)] == 0.0)
    assert np.abs(rec.sum(axis=-1) - 1.0).max() < FP32_TOL
    d_map = None
    if case["stride"]:
        logits2, maps = model.attention_maps(x, m)
        torch.cuda.synchronize()
        assert len(maps) == L and all(t.shape == (B, H, N, N) and t.dtype == torch.float32 and t.is_cuda for t in maps)
        assert torch.equal(logits, logits2)
        rows = z["rows"]
        got = np.stack([t.cpu().numpy() for t in maps])
        assert np.all(got[np.broadcast_to(dead[None, :, None, None, :], got.shape)] == 0.0), "masked key columns must be exactly 0"
        vr = np.broadcast_to(valid[None, :, None, rows, None], z["maps"].shape)
        d_map = np.abs(got[:, :, :, rows, :].astype(np.float64) - z["maps"].astype(np.float64))[vr].max()
        print("%s: maps %.2e" % (case["name"], d_map))
        assert d_map < FP32_TOL, d_map
    assert d_rec < FP32_TOL and d_ent < FP32_TOL, (d_rec, d_ent)


# ---- 2. per-kernel parity -------------------------------------------------------------------------------------------
def _probs(vsa, q, k, mask, want=("maps", "received", "entropy")):
    lib = vsa._lib.load()
    B, H, T, dh = q.shape
    out = {n: None for n in ("maps", "received", "entropy")}
    if "maps" in want:
        out["maps"] = torch.full((B, H, T, T), float("nan"), device=q.device)
    if "received" in want:
        out["received"] = torch.full((B, H, T), float("nan"), device=q.device)
    if "entropy" in want:
        out["entropy"] = torch.full((B, H, T), float("nan"), device=q.device)
    ws = torch.empty((lib.vs_attention_probs_workspace_bytes(B, H, T),), dtype=torch.uint8, device=q.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    vsa._lib.check(lib.vs_attention_probs_f32(q.data_ptr(), k.data_ptr(), ptr(mask), ptr(out["maps"]), ptr(out["received"]),
                                              ptr(out["entropy"]), B, H, T, dh, 256.0 ** -0.5, ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    return out


def _qkv(B, H, T, dh, seed, gain=3.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((B, H, T, dh), generator=g) * gain
    k = torch.randn((B, H, T, dh), generator=g) * gain
    v = torch.randn((B, H, T, dh), generator=g)
    return q, k, v


@pytest.mark.parametrize("dh", [32, 64, 128, 256])
@pytest.mark.parametrize("T", [1, 31, 33, 65, 97, 130, 320])
def test_probs_kernel_against_float64(vsa, dh, T):
    lib = vsa._lib.load()
    B, H = 2, 2
    q, k, v = _qkv(B, H, T, dh, 1000 + dh + T)
    mask = None
    if T > 1:                                               # video 1 is padded, video 0 has a few holes
        mask = torch.zeros((B, T), dtype=torch.bool)
        mask[1, max(1, (2 * T) // 3):] = True
        mask[0, 1::5] = True
    scale = 256.0 ** -0.5
    s = np.einsum("bhid,bhjd->bhij", q.double().numpy(), k.double().numpy()) * scale
    dead = np.zeros((B, T), dtype=bool) if mask is None else mask.numpy()
    s = np.where(dead[:, None, None, :], -np.inf, s)
    P = np.exp(s - s.max(axis=-1, keepdims=True))
    P /= P.sum(axis=-1, keepdims=True)
    rec64, ent64 = attn_cases.reductions64(P, ~dead)
    dq, dk, dv = q.to(_dev()), k.to(_dev()), v.to(_dev())
    dm = None if mask is None else mask.to(_dev()).view(torch.uint8)
    out = _probs(vsa, dq, dk, dm)
    maps = out["maps"].cpu().numpy().astype(np.float64)
    vq = ~dead
    d_map = np.abs(maps - P)[np.broadcast_to(vq[:, None, :, None], P.shape)].max()
    d_sum = np.abs(maps.sum(axis=-1) - 1.0)[np.broadcast_to(vq[:, None, :], (B, H, T))].max()
    d_ent = np.abs(out["entropy"].cpu().numpy() - ent64)[np.broadcast_to(vq[:, None, :], (B, H, T))].max()
    d_rec = np.abs(out["received"].cpu().numpy() - rec64).max()
    # maps @ v in float64 against the scoring kernel's own output (head dim 256: the kernel the scorer runs there,
    # vs_train_attention_forward without dropout)
    att = torch.empty((B, T, H * dh), device=_dev())
    if dh == 256:
        lse = torch.empty((B, H, T), device=_dev())
        vsa._lib.check(lib.vs_train_attention_forward(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), None if dm is None else dm.data_ptr(),
                                                      att.data_ptr(), lse.data_ptr(), B, H, T, dh, scale, 0, 0, 0.0, _stream()))
    else:
        vsa._lib.check(lib.vs_attention_f32(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), None if dm is None else dm.data_ptr(),
                                            att.data_ptr(), B, H, T, dh, scale, _stream()))
    torch.cuda.synchronize()
    o64 = np.einsum("bhij,bhjd->bihd", maps, v.double().numpy()).reshape(B, T, H * dh)
    d_att = np.abs(att.cpu().numpy() - o64)[np.broadcast_to(vq[:, :, None], o64.shape)].max()
    print("dh %d T %d: map %.2e rowsum %.2e entropy %.2e received %.2e maps@v %.2e" % (dh, T, d_map, d_sum, d_ent, d_rec, d_att))
    assert np.all(maps[np.broadcast_to(dead[:, None, None, :], maps.shape)] == 0.0)
    assert not np.isnan(maps).any()
    assert max(d_map, d_sum, d_ent, d_rec, d_att) < FP32_TOL, (d_map, d_sum, d_ent, d_rec, d_att)


def test_probs_kernel_outputs_are_independent_of_each_other(vsa):
    """any subset of the three outputs gives the bits of the full call"""
    q, k, _ = _qkv(2, 2, 97, 64, 5)
    dq, dk = q.to(_dev()), k.to(_dev())
    full = _probs(vsa, dq, dk, None)
    for want in (("maps",), ("received",), ("entropy",), ("received", "entropy")):
        part = _probs(vsa, dq, dk, None, want)
        for n in want:
            assert torch.equal(part[n], full[n]), (want, n)


# ---- 3. bit-equal logits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["attn_d256_h4_t96_randmask_g4", "attn_d200_h5_t130_g4", "attn_cls_d256_h4_t97_g4",
                                  "attn_d256_h1_t150_pad_g8", "attn_d1024_h8_t97_g4"])
def test_logits_are_the_bits_of_forward(vsa, name):
    case = _case(name)
    sd, x, m, _ = _inputs(vsa, case)
    model = _model(vsa, case, sd)
    with torch.no_grad():
        ref = model(x, m)[0]
    a = model.attention_maps(x, m)[0]
    b = model.attention_summary(x, m)[0]
    with torch.no_grad():
        again = model(x, m)[0]
    torch.cuda.synchronize()
    assert torch.equal(a, ref) and torch.equal(b, ref) and torch.equal(again, ref)
    model.train()                                           # eval semantics whatever model.training is, and it is not flipped
    c = model.attention_summary(x, m)[0]
    assert model.training and torch.equal(c, ref)


# ---- 4. summary consistency -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["attn_d256_h4_t96_randmask_g4", "attn_d256_h1_t150_pad_g8", "attn_cls_d256_h4_t97_g4"])
def test_summary_equals_the_reductions_of_the_maps(vsa, name):
    """measured gap (MI355X): see DESIGN.md, the attention-maps section"""
    case = _case(name)
    sd, x, m, mask = _inputs(vsa, case)
    model = _model(vsa, case, sd)
    _, maps = model.attention_maps(x, m)
    _, received, entropy = model.attention_summary(x, m)
    torch.cuda.synchronize()
    valid = attn_cases.valid_rows(case, mask)
    rec64, ent64 = attn_cases.reductions64(np.stack([t.cpu().numpy() for t in maps]), valid)
    d_rec = np.abs(received.cpu().numpy() - rec64).max()
    d_ent = np.abs(entropy.cpu().numpy() - ent64)[np.broadcast_to(valid[None, :, None, :], ent64.shape)].max()
    print("%s: summary vs float64 reductions of the same call's maps: received %.2e entropy %.2e" % (name, d_rec, d_ent))
    assert d_rec < FP32_TOL and d_ent < FP32_TOL, (d_rec, d_ent)


# ---- 5. determinism and batch independence --------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(vsa):
    case = _case("attn_d256_h4_t96_randmask_g4")
    sd, x, m, _ = _inputs(vsa, case)
    model = _model(vsa, case, sd)
    l1, m1 = model.attention_maps(x, m)
    l2, m2 = model.attention_maps(x, m)
    s1, s2 = model.attention_summary(x, m), model.attention_summary(x, m)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(m1, m2))
    assert all(torch.equal(a, b) for a, b in zip(s1, s2))


@pytest.mark.parametrize("dh", [32, 64, 128, 256])
def test_kernel_results_do_not_depend_on_the_batch(vsa, dh):
    """asserted on the kernel: the Linears upstream pick kernels by row count, so the bits of q and k themselves may
    depend on the batch"""
    B, H, T = 3, 2, 130
    q, k, _ = _qkv(B, H, T, dh, 77 + dh)
    mask = torch.zeros((B, T), dtype=torch.bool)
    mask[0, 100:] = True
    mask[1, 3::7] = True
    dq, dk, dm = q.to(_dev()), k.to(_dev()), mask.to(_dev()).view(torch.uint8)
    full = _probs(vsa, dq, dk, dm)
    for b in range(B):
        one = _probs(vsa, dq[b:b + 1].contiguous(), dk[b:b + 1].contiguous(), dm[b:b + 1].contiguous())
        for n in ("maps", "received", "entropy"):
            assert torch.equal(one[n][0], full[n][b]), (b, n)


# ---- 6. layer selection ----------------------------------------------------------------------------------------------
def test_layer_selection_returns_the_slices_of_the_full_call(vsa):
    case = _case("attn_d256_h4_t320_pad_g1")
    sd, x, m, _ = _inputs(vsa, case)
    model = _model(vsa, case, sd)
    l_all, maps = model.attention_maps(x, m)
    _, rec, ent = model.attention_summary(x, m)
    for layers, idx in (([-1], [3]), ([0, 2], [0, 2]), ([2, 0], [2, 0]), ((1,), [1])):
        l_sel, msel = model.attention_maps(x, m, layers=layers)
        _, r, e = model.attention_summary(x, m, layers=layers)
        torch.cuda.synchronize()
        assert torch.equal(l_sel, l_all) and len(msel) == len(idx)
        assert all(torch.equal(a, maps[i]) for a, i in zip(msel, idx))
        assert torch.equal(r, rec[idx]) and torch.equal(e, ent[idx])
    for bad in ([4], [-5], [0, 0], []):
        with pytest.raises(IndexError):
            model.attention_maps(x, m, layers=bad)


def test_inspect_forward_argument_checks_with_a_handle(vsa):
    lib, L = vsa._lib.load(), vsa._lib
    case = _case("attn_d256_h8_t65_g8")
    sd, x, _, _ = _inputs(vsa, case)
    model = _model(vsa, case, sd)
    h = model._packed_weights(x.device).handle
    B, T = x.shape[:2]
    ws = torch.empty((lib.vs_inspect_workspace_bytes(h, B, T, 0),), dtype=torch.uint8, device=x.device)
    scores = torch.empty((B, T, 1), device=x.device)
    ent = torch.empty((1, B, case["H"], T), device=x.device)
    call = lambda layers, n, maps, rec, en, wsb=ws.numel(): lib.vs_inspect_forward(
        h, x.data_ptr(), None, None, B, T, (C.c_int32 * max(len(layers), 1))(*layers), n, scores.data_ptr(), None, maps, rec, en,
        ws.data_ptr(), wsb, _stream())
    assert call([2], 1, None, None, ent.data_ptr()) == L.VS_ERR_INVALID and b"out of range" in lib.vs_last_error()
    assert call([-1], 1, None, None, ent.data_ptr()) == L.VS_ERR_INVALID and b"out of range" in lib.vs_last_error()
    assert call([1, 0], 2, None, None, ent.data_ptr()) == L.VS_ERR_INVALID and b"ascending" in lib.vs_last_error()
    assert call([0], 1, None, None, None) == L.VS_ERR_INVALID and b"all NULL" in lib.vs_last_error()
    assert call([0], 1, None, None, ent.data_ptr() + 4) == L.VS_ERR_INVALID and b"aligned" in lib.vs_last_error()
    assert call([0], 1, None, None, ent.data_ptr(), 256) == L.VS_ERR_WORKSPACE
    assert call([0], 1, None, None, ent.data_ptr()) == L.VS_OK
    torch.cuda.synchronize()


# ---- 7. mode independence -------------------------------------------------------------------------------------------
def test_modes_do_not_change_the_maps_and_the_maps_do_not_change_the_modes(vsa):
    case = _case("attn_d256_h4_t96_randmask_g4")
    sd, x, m, _ = _inputs(vsa, case)
    plain = _model(vsa, case, sd)
    l0, maps0 = plain.attention_maps(x, m)
    _, rec0, ent0 = plain.attention_summary(x, m)
    for setup in (lambda mm: mm.set_compute_dtype("bf16"), lambda mm: mm.set_latency_mode(), lambda mm: mm.set_compute_dtype("fp16x3")):
        used, untouched = _model(vsa, case, sd), _model(vsa, case, sd)
        setup(used), setup(untouched)
        l1, maps1 = used.attention_maps(x, m)
        _, rec1, ent1 = used.attention_summary(x, m)
        with torch.no_grad():
            f_used, f_untouched = used(x, m), untouched(x, m)
        torch.cuda.synchronize()
        assert torch.equal(l1, l0) and all(torch.equal(a, b) for a, b in zip(maps1, maps0))
        assert torch.equal(rec1, rec0) and torch.equal(ent1, ent0)
        assert torch.equal(f_used[0], f_untouched[0]) and torch.equal(f_used[1], f_untouched[1])


# ---- 8. long videos --------------------------------------------------------------------------------------------------
def test_t8192_summary_never_allocates_the_map(vsa):
    B, T, H, d, L = 2, 8192, 4, 256, 4
    sd = attn_cases.apply_gain(vsa.synth.make_state_dict(d, L, 41, in_features=2048, max_len=8192), 4)
    model = vsa.SimNet(num_heads=H, d_model=d, num_layers=L, sparsity=0.0, dropout=0.3, in_features=2048, pe_len=8192)
    model.load_state_dict(sd, strict=True)
    model = model.to(_dev()).eval()
    x = vsa.synth.make_features(B, T, 42, "randn", in_features=2048).to(_dev())
    model.attention_summary(x[:, :64])                      # packs the weights outside the measured call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    logits, received, entropy = model.attention_summary(x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    # the forward's workspace (10 [B, T, d] fp32 regions), one row constant per (video, head, query), the three results, and
    # 16 MiB for the allocator's rounding
    bound = 10 * B * T * d * 4 + B * H * T * 4 + 2 * L * B * H * T * 4 + B * T * 4 + (16 << 20)
    one_map = B * H * T * T * 4
    print("T=8192: peak %.1f MiB, bound %.1f MiB, one layer's map would be %.1f MiB" % (peak / 2 ** 20, bound / 2 ** 20, one_map / 2 ** 20))
    assert bound < one_map // 8
    assert peak <= bound, (peak, bound)
    rec, ent = received.double().cpu().numpy(), entropy.cpu().numpy()
    assert received.shape == entropy.shape == (L, B, H, T)
    assert np.abs(rec.sum(axis=-1) - 1.0).max() < FP32_TOL, np.abs(rec.sum(axis=-1) - 1.0).max()
    # [0, log T] up to the fp32 rounding of the entropy itself (FP32_TOL, the bar the entropy is held to)
    assert ent.min() >= -FP32_TOL and ent.max() <= math.log(T) + FP32_TOL, (ent.min(), ent.max())
    with torch.no_grad():
        assert torch.equal(logits, model(x)[0])
