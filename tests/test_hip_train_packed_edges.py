"""GPU tests of PACKED RAGGED TRAINING where tests/test_hip_train_packed.py does not reach, at the smallest shapes that do:

A. packed steps on the LDS-tiled GEMM family (VS_SKINNY_ROWS = 0), which the benchmark batch (~24 000 rows) runs and no
   packed test did: the goldens, the dropout steps and the bf16 step rerun under the pin; the A-stationary bf16 MLP GEMMs
   against the tiled ones, bit for bit, on a packed batch.
B. "a video's bits do not depend on the batch it is packed in": with both sides on the tiled family, and ACROSS the two
   families (VS_SKINNY_ROWS = 300: the batch tiled, each video alone skinny); Adam steps whose batches cross the threshold.
C. the attention work list and the keep words at their edges: one batch of 16 videos with lengths at and around 128 / 256
   (owner tiles) and 32 / 64 (keep words), equal tile counts and equal lengths - the kernels alone, the full path reading
   the bit-packed words, and the order of the videos.
D. device lengths that disagree with the host's, through the C ABI, with canaries behind every buffer.

Every bound is one of tests/tolerances.py or of the test mirrored; the float64 references run per video (<= 257 frames)."""
import ctypes as C
import importlib
import math

import pytest
import torch

import torch_ref
import test_hip_train_packed as base
from test_hip_train_packed import (PACKED_DROPOUT_STEPS, _check_against_per_video_float64, _close, _cu, _dev, _i32, _lse_of, _model,
                                   _packed_gates, _packed_masks, _stream, packed_cases, padded_cases_that_can_run_packed)

pytestmark = pytest.mark.gpu

EDGE = [128, 127, 129, 1, 256, 257, 255, 32, 31, 33, 64, 63, 65, 2, 128, 32]        # 16 videos, 1 733 rows


@pytest.fixture
def tiled_gemms(vsa):
    """VS_SKINNY_ROWS = 0: every Linear, dgrad and wgrad on the LDS-tiled gemm_nt_128 forms, whatever the batch size"""
    vsa._lib.set_option("VS_SKINNY_ROWS", 0)
    yield
    vsa._lib.set_option("VS_SKINNY_ROWS", -1)


@pytest.fixture
def threshold_300(vsa):
    """VS_SKINNY_ROWS = 300: batches of more than 300 rows run tiled, batches (and single videos) up to 300 rows skinny"""
    vsa._lib.set_option("VS_SKINNY_ROWS", 300)
    yield
    vsa._lib.set_option("VS_SKINNY_ROWS", -1)


@pytest.fixture
def lp_train_everywhere(vsa):
    vsa._lib.set_option("VS_TRAIN_LP_MIN_ROWS", 0)
    yield
    vsa._lib.set_option("VS_TRAIN_LP_MIN_ROWS", -1)


# ---------------------------------------------------------------------------------------------
# A. packed steps on the tiled GEMMs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", packed_cases(), ids=lambda c: c["name"])
def test_packed_gradients_match_reference_golden_on_tiled_gemms(vsa, case, tiled_gemms):
    """the packed goldens as they are under the pin: same float64 vectors, same bounds (no fc1 pre-activation of these inputs
    falls on the other side of the ReLU on the tiled GEMMs either, so no explicit-gate model is needed)"""
    base.test_packed_gradients_match_reference_golden(vsa, case)


@pytest.mark.parametrize("case", padded_cases_that_can_run_packed(), ids=lambda c: c["name"])
def test_padded_goldens_run_packed_on_tiled_gemms(vsa, case, tiled_gemms):
    base.test_padded_goldens_run_packed(vsa, case)


@pytest.mark.parametrize("H,d,L,lengths,p,p_embed", PACKED_DROPOUT_STEPS)
def test_packed_training_step_with_dropout_on_tiled_gemms(vsa, H, d, L, lengths, p, p_embed, tiled_gemms):
    """the fc1 + ReLU + dropout epilogue, the gated fc2 dgrad and the dgrads adding the residual gradient, on a packed batch"""
    base.test_packed_training_step_with_dropout_matches_explicit_mask_model(vsa, H, d, L, lengths, p, p_embed)


def test_packed_bf16_training_gradients_on_tiled_gemms(vsa, lp_train_everywhere, tiled_gemms):
    """the bf16 / fp16 step of the packed suite, rerun under the pin"""
    base.test_packed_bf16_training_gradients_within_the_low_precision_tolerance(vsa, None)


@pytest.mark.parametrize("d,lengths", [(256, [129, 64, 33, 1]), (512, [97, 64])])
def test_packed_a_stationary_mlp_gemms_equal_the_tiled_ones_bit_for_bit(vsa, lp_train_everywhere, d, lengths):
    """test_hip_train.test_a_stationary_mlp_gemms_equal_the_tiled_ones_bit_for_bit on a packed batch (B = 1, T = Mtot rows,
    the gathered positional rows, the [H][Mtot][dh] QKV epilogue): VS_LP_MLP_UNFUSED = 2 (vst_gemm_rows16 at every batch
    size) and = 1 (the tiled kernels) give the same logits, hidden state, dx and gradients; dropout 0.3, one seed."""
    res = {}
    x = torch.randn(sum(lengths), 1024, generator=torch.Generator().manual_seed(1))
    try:
        for tiled in (1, 0):
            vsa._lib.set_option("VS_LP_MLP_UNFUSED", 1 if tiled else 2)
            m = _model(vsa, dict(H=4, d=d, L=2, wseed=3), dropout=0.3).set_train_dtype("bf16")
            xd = x.to(_dev()).requires_grad_(True)
            torch.manual_seed(5)
            pred, hid = m.forward_packed_train(xd, lengths)
            ((pred ** 2).mean() + 1e-3 * hid.sum()).backward()
            assert m.last_train_dtype == "bf16"
            rows16 = (int(vsa._lib.load().vs_train_last_format()) & 16) != 0
            assert rows16 == (not tiled), "the switch did not select the GEMM form"
            res[tiled] = [("pred", pred.detach().clone()), ("hidden", hid.detach().clone()), ("dx", xd.grad.clone())] + \
                         [(n, q.grad.clone()) for n, q in m.named_parameters()]
    finally:
        vsa._lib.set_option("VS_LP_MLP_UNFUSED", -1)
    for (n, a), (_n, b) in zip(res[1], res[0]):
        assert torch.isfinite(a).all() and torch.equal(a, b), n


# ---------------------------------------------------------------------------------------------
# B. batch independence within and across the GEMM families
# ---------------------------------------------------------------------------------------------
INDEPENDENCE = [(4, 256, 2, [211, 129, 33, 70]), (4, 512, 1, [150, 97, 64, 1])]


def _forward_and_dx(vsa, m, x, R, lengths, L):
    """logits, hidden state, every layer's lse2 and dx of one packed batch.  The loss is a sum over rows (sum pred^2 + 1e-3
    sum hidden * R), so a row's loss gradient is a function of that row's outputs alone and dx can be compared by slices."""
    xd = x.to(_dev()).requires_grad_(True)
    pred, hid = m.forward_packed_train(xd, lengths)
    lse = [_lse_of(vsa, m, pred, lengths, l) for l in range(L)]
    ((pred ** 2).sum() + 1e-3 * (hid * R.to(_dev())).sum()).backward()
    return [pred.detach(), hid.detach()] + lse + [xd.grad]


def _slice(tensors, L, sl):
    """rows sl of (pred, hidden, lse2 per layer [H, Mtot], dx)"""
    return [t[:, sl] if 2 <= i < 2 + L else t[sl] for i, t in enumerate(tensors)]


@pytest.mark.parametrize("H,d,L,lengths", INDEPENDENCE)
def test_a_videos_bits_do_not_depend_on_the_batch_on_tiled_gemms(vsa, H, d, L, lengths, tiled_gemms):
    """both sides on the tiled family: each video alone gives the bits of its slice of the batch (logits, hidden state, lse2
    of every layer, dx)"""
    m = _model(vsa, dict(H=H, d=d, L=L, wseed=5))
    x = torch.randn(sum(lengths), 1024, generator=torch.Generator().manual_seed(2))
    R = torch.randn(sum(lengths), d, generator=torch.Generator().manual_seed(3))
    whole, cu = _forward_and_dx(vsa, m, x, R, lengths, L), _cu(lengths)
    names = ["logits", "hidden"] + ["lse2 of layer %d" % l for l in range(L)] + ["dx"]
    for b, t in enumerate(lengths):
        sl = slice(cu[b], cu[b + 1])
        alone = _forward_and_dx(vsa, m, x[sl], R[sl], [t], L)
        for n, a, w in zip(names, alone, _slice(whole, L, sl)):
            assert torch.isfinite(a).all() and torch.equal(a, w), (b, n)


@pytest.mark.parametrize("H,d,L,lengths", INDEPENDENCE)
def test_a_videos_bits_across_the_gemm_families(vsa, H, d, L, lengths, threshold_300):
    """VS_SKINNY_ROWS = 300 lies between the longest video and the batch: the batch runs the tiled GEMMs (gemm_nt_128), every
    video alone the skinny ones (skinny2_gemm; a kernel trace shows the two families) - and still each video alone gives the
    bits of its slice of the batch, so "a video's bits do not depend on the batch it is packed in" (include/vs_train.h,
    DESIGN section 23) holds without a qualification about the batch size.  This pins that: a change to the summation order
    of one family alone fails here."""
    assert max(lengths) <= 300 < sum(lengths)
    m = _model(vsa, dict(H=H, d=d, L=L, wseed=5))
    x = torch.randn(sum(lengths), 1024, generator=torch.Generator().manual_seed(2))
    R = torch.randn(sum(lengths), d, generator=torch.Generator().manual_seed(3))
    whole, cu = _forward_and_dx(vsa, m, x, R, lengths, L), _cu(lengths)
    names = ["logits", "hidden"] + ["lse2 of layer %d" % l for l in range(L)] + ["dx"]
    worst = {}
    for b, t in enumerate(lengths):
        sl = slice(cu[b], cu[b + 1])
        alone = _forward_and_dx(vsa, m, x[sl], R[sl], [t], L)
        for n, a, w in zip(names, alone, _slice(whole, L, sl)):
            assert torch.isfinite(a).all(), (b, n)
            worst[n] = max(worst.get(n, 0.0), (a.double() - w.double()).abs().max().item())
            assert torch.equal(a, w), (b, n, worst[n])
    print("batch (tiled GEMMs) against each video alone (skinny GEMMs), largest |difference|: %s" % worst)


def _native_adam_step(vsa, harness, m, opt, scaler, x, target, lengths, d, L, tseed):
    """One harness.train_step_packed on one batch.  Returns what the float64 checker needs: the dropout seed the step drew,
    its gates (read from the activation record before the backward frees it), logits, loss and the unscaled gradients."""
    torch.manual_seed(tseed)
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    torch.manual_seed(tseed)
    seen = {}
    inner = m.forward_packed_train

    def recording(feature, lens):
        pred, hid = inner(feature, lens)
        seen["pred"], seen["gates"] = pred.detach().clone(), _packed_gates(vsa, m, pred, lens, d, L)
        return pred, hid
    m.forward_packed_train = recording
    try:
        xd = x.to(_dev()).requires_grad_(True)          # already on the device: the step's .to(device) hands this leaf on
        scale = scaler.get_scale()
        loss = harness.train_step_packed(m, opt, [(xd, target, lengths)], scaler, _dev())
    finally:
        del m.forward_packed_train
    assert scaler.get_scale() == scale, "the step overflowed"
    # the native Adam takes the scale as a device scalar and leaves .grad scaled (a power of two: the division is exact)
    grads = {"x": xd.grad / scale}
    grads.update({k: prm.grad / scale for k, prm in m.named_parameters()})
    return seed, seen["gates"], seen["pred"], loss, grads


def test_packed_batches_crossing_the_skinny_threshold_between_native_adam_steps(vsa, threshold_300):
    """test_hip_train_at_scale.test_batches_crossing_the_skinny_threshold_between_adam_steps on packed batches at small
    shapes: four steps of harness.train_step_packed with the native Adam (write-through into the packed weights),
    alternating 200 rows (skinny) and 443 rows (tiled), dropout 0.3.  The transposed and fragment-major weight copies each
    family reads must follow the parameters: every step's gradients against float64 at the parameters current for it."""
    harness = importlib.import_module("video-summarization_amd.harness")
    H, d, L, p = 4, 256, 2, 0.3
    m = _model(vsa, dict(H=H, d=d, L=L, wseed=41), dropout=p)
    opt = vsa.Adam(m.parameters(), lr=1e-3).attach(m)
    scaler = torch.amp.GradScaler("cuda")
    for i, lengths in enumerate([[129, 71], [211, 129, 33, 70], [129, 71], [211, 129, 33, 70]]):
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        M = sum(lengths)
        x = torch.randn(M, 1024, generator=torch.Generator().manual_seed(50 + i))
        target = torch.rand(M, generator=torch.Generator().manual_seed(60 + i))
        seed, gates, pred, loss, grads = _native_adam_step(vsa, harness, m, opt, scaler, x, target, lengths, d, L, 70 + i)
        masks = _packed_masks(vsa, lengths, d, H, L, seed, p, 0.0)
        _check_against_per_video_float64(sd, x, target, lengths, H, p, 0.0, masks, gates, torch.tensor(loss), pred, grads, hidden_w=0.0)
        moved = max((v.detach().cpu() - sd[k]).abs().max().item() for k, v in m.state_dict().items())
        assert moved > 1e-4, "the optimizer did not step"


# ---------------------------------------------------------------------------------------------
# C. attention tile and keep-word edges, many videos
# ---------------------------------------------------------------------------------------------
def _attention_packed(vsa, q, k, v, dO, lengths, H, dh, scale, seed, site, p):
    """out [M, d], lse2 [H, M], dqkv [M, 3d] of the packed attention kernels; outputs prefilled with NaN"""
    lib = vsa._lib.load()
    B, M, d = len(lengths), sum(lengths), H * dh
    host, dl = _i32(lengths), torch.tensor(lengths, dtype=torch.int32, device=_dev())
    ws = torch.empty(lib.vs_train_attention_packed_scratch_bytes(host, B, H), dtype=torch.uint8, device=_dev())
    out = torch.full((M, d), float("nan"), device=_dev())
    lse = torch.full((H, M), float("nan"), device=_dev())
    dqkv = torch.full((M, 3 * d), float("nan"), device=_dev())
    vsa._lib.check(lib.vs_train_attention_forward_packed(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), host,
                                                         dl.data_ptr(), B, H, dh, scale, seed, site, p, ws.data_ptr(), ws.numel(), _stream()))
    vsa._lib.check(lib.vs_train_attention_backward_packed(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dO.data_ptr(),
                                                          lse.data_ptr(), dqkv.data_ptr(), host, dl.data_ptr(), B, H, dh, scale, seed, site, p,
                                                          ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    return out, lse, dqkv


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("H,dh", [(2, 32), (2, 64), (2, 128), (1, 256)])
def test_packed_attention_kernels_at_tile_and_keep_word_edges(vsa, H, dh, p):
    """test_hip_train_packed.test_packed_attention_forward_and_backward_kernels (its bounds, its float64 checker with the
    library's keep mask, its NaN prefill) on EDGE; and, dropout off, every video's out / lse2 / dqkv are the bits of the
    same video run as a one-video packed batch (with p > 0 the dropout row key holds head * Mtot + row: no such identity)."""
    lib = vsa._lib.load()
    lengths = EDGE
    B, M, d, cu = len(lengths), sum(lengths), H * dh, _cu(lengths)
    scale, seed, site = d ** -0.5, 0x1234567887654321, 7
    g = torch.Generator().manual_seed(100 + M + dh)
    q, k, v = (torch.randn(H, M, dh, generator=g, dtype=torch.float64) for _ in range(3))
    dO = torch.randn(M, d, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    keep = None
    if p > 0:
        kd = torch.empty(H * sum(t * t for t in lengths), dtype=torch.uint8, device=_dev())
        vsa._lib.check(lib.vs_train_dropout_mask_attention_packed(kd.data_ptr(), _i32(lengths), B, H, seed, site, p, _stream()))
        kd, off, keep = kd.cpu(), 0, []
        for t in lengths:
            keep.append(kd[off: off + H * t * t].view(1, H, t, t))
            off += H * t * t
        rate = kd.double().mean().item()
        assert abs(rate - (1 - p)) < 5 * math.sqrt(p * (1 - p) / kd.numel()), rate
    qd, kd_, vd, dOd = (t.float().to(_dev()).contiguous() for t in (q, k, v, dO))
    out, lse, dqkv = _attention_packed(vsa, qd, kd_, vd, dOd, lengths, H, dh, scale, seed, site, p)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()       # every row written
    for b, t in enumerate(lengths):
        sl = slice(cu[b], cu[b + 1])
        qb, kb, vb = (u[:, sl][None].clone().requires_grad_(True) for u in (q, k, v))
        want, lse2 = torch_ref.attention_with_mask(qb, kb, vb, None, scale, None if keep is None else keep[b], p)
        want.backward(dO[sl][None])
        _close(out[sl], want[0], "attention out, video %d" % b)
        assert (lse[:, sl].cpu().double() - lse2.detach()[0]).abs().max().item() < 1e-4
        tok = lambda gr: gr[0].permute(1, 0, 2).reshape(t, d)       # noqa: E731  head-major grad -> token-major
        _close(dqkv[sl, :d], tok(qb.grad), "dq, video %d" % b)
        _close(dqkv[sl, d:2 * d], tok(kb.grad), "dk, video %d" % b)
        _close(dqkv[sl, 2 * d:], tok(vb.grad), "dv, video %d" % b)
        if p == 0.0:
            o1, l1, g1 = _attention_packed(vsa, qd[:, sl].contiguous(), kd_[:, sl].contiguous(), vd[:, sl].contiguous(),
                                           dOd[sl].contiguous(), [t], H, dh, scale, seed, site, p)
            assert torch.equal(o1, out[sl]) and torch.equal(l1, lse[:, sl]) and torch.equal(g1, dqkv[sl]), b


@pytest.mark.parametrize("H,d,L,p,p_embed", [(4, 256, 1, 0.3, 0.25), (4, 512, 1, 0.3, 0.0)])
def test_packed_training_step_reads_the_keep_words_at_their_edges(vsa, H, d, L, p, p_embed):
    """One training step with dropout on EDGE[:9] (videos of exactly 128 / 256 / 32 rows and their neighbours): the full path
    reads the bit-packed keep words (attn_dropout_bits<true>, the bo offsets), the per-video float64 checker the byte masks
    the library exports - a wrong offset or a wrong word at a 32-key edge is a gradient error.  The dropout test's checks."""
    lengths = EDGE[:9]
    sd = vsa.synth.make_state_dict(d, L, 21)
    m = vsa.SimNet(num_heads=H, d_model=d, num_layers=L, sparsity=p_embed, dropout=p)
    m.load_state_dict(sd, strict=True)
    m = m.to(_dev()).train()
    M = sum(lengths)
    x = torch.randn(M, 1024, generator=torch.Generator().manual_seed(22))
    target = torch.rand(M, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(77)
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())        # what forward_packed_train will draw
    torch.manual_seed(77)
    xd = x.to(_dev()).requires_grad_(True)
    pred, hidden = m.forward_packed_train(xd, lengths)
    loss = vsa.mse_packed_loss(pred, target.to(_dev()), lengths) + 1e-3 * hidden.sum()
    gates = _packed_gates(vsa, m, pred, lengths, d, L)
    loss.backward()
    torch.cuda.synchronize()
    masks = _packed_masks(vsa, lengths, d, H, L, seed, p, p_embed)
    for name, km in masks.items():
        for part in (km if isinstance(km, list) else [km]):
            pp = p_embed if name == "embed" else p
            rate, n = part.double().mean().item(), part.numel()
            assert abs(rate - (1 - pp)) < 5 * math.sqrt(pp * (1 - pp) / n), (name, rate, n)
    grads = {"x": xd.grad}
    grads.update({k: prm.grad for k, prm in m.named_parameters()})
    _check_against_per_video_float64(sd, x, target, lengths, H, p, p_embed, masks, gates, loss, pred, grads)


def _order_independence(vsa):
    lengths, cu = EDGE, _cu(EDGE)
    m = _model(vsa, dict(H=4, d=256, L=2, wseed=5))
    x = torch.randn(sum(lengths), 1024, generator=torch.Generator().manual_seed(2))
    pred, hid = m.forward_packed_train(x.to(_dev()), lengths)
    order = list(range(len(lengths)))[::-1]
    xr = torch.cat([x[cu[b]:cu[b + 1]] for b in order])
    rl = [lengths[b] for b in order]
    rcu = _cu(rl)
    pr, hr = m.forward_packed_train(xr.to(_dev()), rl)
    assert torch.isfinite(pred).all() and torch.isfinite(hid).all()
    for i, b in enumerate(order):
        a, r = slice(cu[b], cu[b + 1]), slice(rcu[i], rcu[i + 1])
        assert torch.equal(pred[a], pr[r]) and torch.equal(hid[a], hr[r]), b


def test_the_order_of_the_videos_does_not_change_a_videos_bits(vsa):
    """EDGE and EDGE reversed, dropout off: the plan's longest-first ordering (with ties among equal tile counts and equal
    lengths) and the row offsets change, each video's logits and hidden state do not."""
    _order_independence(vsa)


def test_the_order_of_the_videos_does_not_change_a_videos_bits_on_tiled_gemms(vsa, tiled_gemms):
    _order_independence(vsa)


# ---------------------------------------------------------------------------------------------
# D. device lengths that disagree with the host's
# ---------------------------------------------------------------------------------------------
CANARY = 0xA5


class _Guarded:
    """`nbytes` bytes for the library followed by `slack` canary bytes, in one allocation"""

    def __init__(self, nbytes, slack):
        self.n = nbytes
        self.buf = torch.full((nbytes + slack,), CANARY, dtype=torch.uint8, device=_dev())
        assert self.buf.data_ptr() % 256 == 0

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.n:] == CANARY).all().item())

    def floats(self, count):
        return self.buf[:4 * count].view(torch.float32)


@pytest.mark.parametrize("host,device,p", [([100, 100], [200, 100], 0.3), ([129, 64], [64, 64], 0.3), ([129, 64], [64, 64], 0.0),
                                           ([64, 64], [64, 300], 0.0), ([96, 32, 32, 32], [96, 96, 32, 32], 0.3)])
def test_device_lengths_that_disagree_with_the_hosts_stay_inside_what_the_host_sized(vsa, host, device, p):
    """vs_train_forward_packed / _backward_packed with lengths_dev != lengths.  plan_packed_train cuts a length at the host's
    longest video and the rows at Mtot, gives a video whose keep words would not fit the host-sized area length 0 and marks
    the unused tail of the work list, so nothing is written outside what the host sized.  The test owns every buffer: each
    is followed by canary bytes, at least as many as the DEVICE lengths would need, so a missing clamp changes a canary and
    never leaves the allocation.  [100, 100] / [200, 100]: 200 rows of one video need 1 400 keep words per head, the record
    has 800 (the plan without its bounds wrote 2 400 bytes behind the record here); [129, 64] / [64, 64]: fewer owner tiles
    than the host's; [64, 64] / [64, 300]: the sum exceeds Mtot; [96, 32, 32, 32] / [96, 96, 32, 32]: no length above the
    host's longest, no row beyond Mtot, and still 576 + 64 words where the host sized 384 - the word bound alone.  One
    model layer, so the keep words are the record's last field."""
    lib = vsa._lib.load()
    H, d, L = 4, 256, 1
    m = _model(vsa, dict(H=H, d=d, L=L, wseed=3))
    handle = m._packed_weights(_dev()).handle
    simnet = importlib.import_module("video-summarization_amd.simnet")
    B, M = len(host), sum(host)
    hl, big = _i32(host), _i32([max(a, b) for a, b in zip(host, device)])        # `big` sizes the slack only
    saved_n, ws_n = lib.vs_train_saved_bytes_packed(handle, hl, B), lib.vs_train_workspace_bytes_packed(handle, hl, B)
    slack_saved, slack_ws = lib.vs_train_saved_bytes_packed(handle, big, B), lib.vs_train_workspace_bytes_packed(handle, big, B)
    assert 0 < saved_n <= slack_saved and 0 < ws_n <= slack_ws
    Mbig = sum(max(a, b) for a, b in zip(host, device))
    x = torch.randn(M, 1024, generator=torch.Generator().manual_seed(1)).to(_dev())
    d_scores = torch.randn(M, 1, generator=torch.Generator().manual_seed(2)).to(_dev())
    cfg = vsa._lib.DropoutCfg(0.0, p, 0x5eed, 0, 0)

    def call(lengths_dev):
        """forward + backward on fresh guarded buffers; returns (scores, hidden, dx, gradients) and the guards"""
        dl = torch.tensor(lengths_dev, dtype=torch.int32, device=_dev())
        saved, ws = _Guarded(saved_n, slack_saved), _Guarded(ws_n, slack_ws)
        scores, hidden, dx = _Guarded(4 * M, 4 * Mbig), _Guarded(4 * M * d, 4 * Mbig * d), _Guarded(4 * M * 1024, 4 * Mbig * 1024)
        grads, G, _finish = simnet._grad_destinations(m, _dev())
        rc = lib.vs_train_forward_packed(handle, x.data_ptr(), hl, dl.data_ptr(), B, C.byref(cfg), scores.ptr(), hidden.ptr(),
                                         saved.ptr(), saved_n, ws.ptr(), ws_n, _stream())
        assert rc == vsa._lib.VS_OK, lib.vs_last_error()
        rc = lib.vs_train_backward_packed(handle, x.data_ptr(), hl, dl.data_ptr(), B, C.byref(cfg), d_scores.data_ptr(), None,
                                          saved.ptr(), saved_n, C.byref(G), dx.ptr(), ws.ptr(), ws_n, _stream())
        assert rc == vsa._lib.VS_OK, lib.vs_last_error()
        torch.cuda.synchronize()
        guards = dict(saved=saved, workspace=ws, scores=scores, hidden=hidden, dx=dx)
        return [scores.floats(M).clone(), hidden.floats(M * d).clone(), dx.floats(M * 1024).clone()] + [g.clone() for g in grads], guards

    fresh, guards = call(host)
    assert all(torch.isfinite(t).all() for t in fresh) and all(g.intact() for g in guards.values())
    odd, guards = call(device)
    broken = [name for name, g in guards.items() if not g.intact()]
    assert not broken, "bytes behind %s were written (device lengths %r, host lengths %r)" % (broken, device, host)
    if device[0] == host[0]:        # the first video: same length, same offset - the bits of the consistent call
        assert torch.equal(odd[0][:host[0]], fresh[0][:host[0]])
    again, guards = call(host)
    assert all(g.intact() for g in guards.values())
    for a, b in zip(again, fresh):
        assert torch.equal(a, b)
