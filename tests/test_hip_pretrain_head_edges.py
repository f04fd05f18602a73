"""GPU tests of the PRETRAINING LOSS HEAD (csrc/vs_pretrain_kernels.hip; include/vs_train.h: vs_pretrain_head_forward / _backward
and their _packed counterparts) at the edges its other tests leave out: chunk and stride edges of T, all four feature widths,
interior masks with a masked chunk and a masked frame 0, scores past the fp32 exp range, a video with every frame masked,
more than 64 packed videos (the carry of pk_locate's scan), the two kernel families against each other bit for bit, and
guard bands round every buffer of the padded C entries.

Checker: the float64 restatements of tests/pretrain_ref.py on fp32-representable inputs.  Bars: those of tests/test_pretrain.py,
unchanged - each loss within 2e-6 * max(1, |want|), each gradient within 2e-5 * max|want| + 1e-9, gradients of
loss + 0.5 center + repel.  An fp32 torch restatement of the same formulas stays within 1.3e-7 (losses) and 1.1e-6 (gradients)
of float64 on every case below except the +40 score shift, where the gradients are at 2.3e-6.
Every case runs on the latency GEMMs and on the tiled ones."""
import ctypes as C
import importlib

import pytest
import torch

from pretrain_ref import head_reference, head_reference_packed, tiled_gemms      # noqa: F401  (tiled_gemms: a fixture)

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
TEMP = 0.4
GUARD = 4096
UP = (1.0, 0.5, 1.0)                                                  # pretrain.py:62
LOSSES = ("distillation", "centering", "repelling")
GRADS = ("d_hidden", "d_logits", "d_weight", "d_bias")
_WANT = {}


@pytest.fixture(params=["latency_gemms", "tiled_gemms"])
def gemms(request):
    """every case twice: video_transform on the GEMMs its row count picks, and with VS_SKINNY_ROWS = 0 (tiled_gemms)"""
    if request.param == "tiled_gemms":
        request.getfixturevalue("tiled_gemms")


def _heads():
    m = importlib.import_module("video-summarization_amd.pretrain")
    return m._PretrainHead, m._PretrainHeadPacked


def _check(tag, got_losses, got_grads, want_losses, want_grads):
    """test_pretrain.py's bars; every figure is printed before it is asserted"""
    for i, name in enumerate(LOSSES):
        g, w = float(got_losses[i]), float(want_losses[i])
        print("%s %s: %.9f (float64 %.9f)" % (tag, name, g, w))
        assert abs(g - w) < 2e-6 * max(1.0, abs(w)), (tag, name, g, w)
    for a, r, name in zip(got_grads, want_grads, GRADS):
        assert a.shape == r.shape, (tag, name, a.shape, r.shape)
        err = (a.double().cpu() - r).abs().max().item()
        scale = r.abs().max().item()
        print("%s %s: err %.3e, max %.3e" % (tag, name, err, scale))
        assert err <= 2e-5 * scale + 1e-9, "%s %s: err %.3e, max %.3e" % (tag, name, err, scale)


def _inputs(seed, rows, d, Fo, B, shift=0.0):
    """hidden, logits, weight, bias and vid in float64 with fp32-representable values (drawn in fp32): the kernels and the
    checker see the same numbers.  rows: the leading shape of hidden / logits, (B, T) or (Mtot,)."""
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(*rows, d, generator=g)
    logits = torch.randn(*rows, 1, generator=g) + shift
    vid = torch.randn(B, Fo, generator=g)
    W = torch.randn(Fo, d, generator=g) / d ** 0.5
    bias = 0.1 * torch.randn(Fo, generator=g)
    return [t.double() for t in (hidden, logits, W, bias)], vid.double()


def _mask(vsa, B, T, kind):
    """"tail": the suffix masks of test_pretrain.py.  "interior": a random mask with frame 0 valid in video 0 and masked in
    video 1, a valid frame in every video and, from T = 129, video 0's chunk 64..127 masked as a whole."""
    if kind is None:
        return None
    if kind == "tail":
        mask = torch.zeros(B, T, dtype=torch.bool)
        for i in range(B):
            mask[i, T - 7 * i - 3:] = True
        return mask
    mask = vsa.synth.random_mask(B, T, seed=1000 + T).clone()          # never masks frame 0
    mask[1, 0] = True
    if T >= 129:
        mask[0, 64:128] = True
    for i in range(B):
        if mask[i].all():
            mask[i, T - 1] = False
    assert not mask[0, 0] and mask[1, 0] and (~mask).any(dim=1).all() and mask.any()
    return mask


# ---------------------------------------------------------------------------------------------
# 1. the padded head against float64 at its edges
# ---------------------------------------------------------------------------------------------
def _pid(c):
    B, T, d, Fo, pen, kind, temp, shift = c
    return "B%d-T%d-d%d-F%d-%s-%s-temp%g%s" % (B, T, d, Fo, pen, kind or "nomask", temp, "-shift%g" % shift if shift else "")


def _padded_want(vsa, c):
    """float64 inputs, mask, losses and gradients of a padded case: computed once, shared by the two GEMM settings, never modified"""
    if c not in _WANT:
        B, T, d, Fo, pen, kind, temp, shift = c
        inputs, vid = _inputs(B * T * 3 + d + Fo, (B, T), d, Fo, B, shift)
        mask = _mask(vsa, B, T, kind)
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        want = head_reference(leaves[0], leaves[1], vid, mask, leaves[2], leaves[3], temp, pen)
        sum(u * w for u, w in zip(UP, want)).backward()
        _WANT[c] = (inputs, vid, mask, [w.item() for w in want], [t.grad for t in leaves])
    return _WANT[c]


def _run_padded(vsa, c, mask_as=None):
    B, T, d, Fo, pen, kind, temp, shift = c
    inputs, vid, mask, _, _ = _padded_want(vsa, c)
    dl = [t.float().to(DEV).requires_grad_(True) for t in inputs]
    m = None if mask is None else (mask if mask_as is None else mask.to(mask_as)).to(DEV)
    got = _heads()[0].apply(dl[0], dl[1], vid.float().to(DEV), m, dl[2], dl[3], temp, pen == "entropy")
    sum(u * g for u, g in zip(UP, got)).backward()
    torch.cuda.synchronize()
    return got.detach().cpu(), [t.grad for t in dl]


def _padded_case(vsa, c):
    _, _, _, want_losses, want_grads = _padded_want(vsa, c)
    got_losses, got_grads = _run_padded(vsa, c)
    _check(_pid(c), got_losses, got_grads, want_losses, want_grads)
    return got_losses, got_grads


# T = 1..5: chunk waves without a frame, waves idle after `t += 4`; 63..65, 127..129: the 64-frame chunk from both sides;
# 257: softmax_stats strides twice; 1025: five times, 17 chunks
EDGE_T = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 1025)
EDGE_CASES = [(3, T, 128, 256, pen, "interior" if T >= 4 else None, TEMP, 0.0) for T in EDGE_T for pen in ("entropy", "norm")]
# all four instantiations of the five kernels: tail mask, interior mask (with a masked chunk) and no mask
WIDTH_CASES = [(2, 130, 64, Fo, pen, kind, TEMP, 0.0) for Fo in (256, 512, 768, 1024)
               for pen, kind in (("entropy", "tail"), ("norm", "interior"), ("entropy" if Fo % 512 else "norm", None))]
# s / temp = 100 at the +40 shift: expf overflows without the max subtraction of softmax_stats; a sharp and a flat softmax
SOFTMAX_CASES = [(2, 150, 64, 512, pen, "tail", TEMP, 40.0) for pen in ("entropy", "norm")]
SOFTMAX_CASES += [(2, 150, 64, 512, pen, "interior", temp, 0.0) for temp in (0.1, 1.0) for pen in ("entropy", "norm")]


@gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=_pid)
def test_padded_head_at_chunk_and_stride_edges(vsa, case, gemms):
    _, got_grads = _padded_case(vsa, case)
    if case[1] == 1:
        # one frame: w = 1 and R = w * dw, so the kernel's w * (dw - R) is exactly 0, as is the analytic gradient
        assert torch.count_nonzero(got_grads[1]).item() == 0, got_grads[1]


@gpu
@pytest.mark.parametrize("case", WIDTH_CASES, ids=_pid)
def test_padded_head_at_every_feature_width(vsa, case, gemms):
    _padded_case(vsa, case)


@gpu
@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=_pid)
def test_padded_head_softmax_is_stable_and_follows_temp(vsa, case, gemms):
    _padded_case(vsa, case)


@gpu
@pytest.mark.parametrize("pen", ["entropy", "norm"])
def test_mask_dtype_does_not_change_a_bit(vsa, pen, gemms):
    """the same key mask as bool, as uint8 and as a float tensor through _PretrainHead.apply"""
    c = (3, 65, 64, 256, pen, "interior", TEMP, 0.0)
    l0, g0 = _run_padded(vsa, c)
    assert all(torch.isfinite(g).all() for g in g0) and g0[0].abs().max().item() > 0
    for dtype in (torch.uint8, torch.float32):
        l1, g1 = _run_padded(vsa, c, mask_as=dtype)
        assert torch.equal(l0, l1), (dtype, l0, l1)
        for a, b, name in zip(g0, g1, GRADS):
            assert torch.equal(a, b), (dtype, name)


@gpu
@pytest.mark.parametrize("pen", ["entropy", "norm"])
def test_each_loss_routes_its_own_gradient(vsa, pen, gemms):
    """d_losses = each unit vector in turn against the float64 gradient of that loss alone: in the weighted sum a wrong
    coefficient on one term can hide behind another."""
    B, T, d, Fo = 3, 65, 64, 256
    inputs, vid = _inputs(9165, (B, T), d, Fo, B)
    mask = _mask(vsa, B, T, "interior")
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    want = head_reference(leaves[0], leaves[1], vid, mask, leaves[2], leaves[3], TEMP, pen)
    dl = [t.float().to(DEV).requires_grad_(True) for t in inputs]
    got = _heads()[0].apply(dl[0], dl[1], vid.float().to(DEV), mask.to(DEV), dl[2], dl[3], TEMP, pen == "entropy")
    for i, name in enumerate(LOSSES):
        wg = torch.autograd.grad(want[i], leaves, retain_graph=True, allow_unused=True)
        wg = [torch.zeros_like(t) if g is None else g for g, t in zip(wg, leaves)]      # centering does not see hidden / weight / bias
        unit = torch.zeros(3, device=DEV)
        unit[i] = 1.0
        gg = torch.autograd.grad(got, dl, grad_outputs=unit, retain_graph=True)
        torch.cuda.synchronize()
        _check("%s alone (%s)" % (name, pen), got.detach().cpu(), gg, [w.item() for w in want], wg)
        assert any(g.abs().max().item() > 0 for g in wg)


# ---------------------------------------------------------------------------------------------
# the C entries with every device buffer carved out of a canary-filled allocation
# ---------------------------------------------------------------------------------------------
class _Band:
    """nbytes, 256-byte aligned, with at least GUARD bytes of 0xA5 on either side; nan: the bytes inside start as fp32 NaN"""

    def __init__(self, nbytes, nan=False):
        self.n = int(nbytes)
        self.whole = torch.full((2 * GUARD + self.n + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        self.off = GUARD + (-(self.whole.data_ptr() + GUARD)) % 256
        assert self.off >= GUARD and self.whole.numel() - self.off - self.n >= GUARD and self.ptr() % 256 == 0
        if nan:
            self.floats().fill_(float("nan"))

    def ptr(self):
        return self.whole.data_ptr() + self.off

    def floats(self):
        return self.whole[self.off:self.off + self.n].view(torch.float32)

    def intact(self):
        return bool((self.whole[:self.off] == 0xA5).all()) and bool((self.whole[self.off + self.n:] == 0xA5).all())


def _c_padded_head(vsa, hidden, logits, mask, vid, W, bias, temp, entropy, up=UP):
    """vs_pretrain_head_forward + _backward as pretrain.py calls them, on carved buffers: feats, head_state of exactly
    vs_pretrain_head_state_bytes, losses, the four gradients and the workspace of exactly vs_pretrain_head_workspace_bytes.
    Returns the bands after asserting VS_OK and intact canaries."""
    lib, L = vsa._lib.load(), vsa._lib
    B, T, d = hidden.shape
    Fo = W.shape[0]
    hidden, logits, vid, W, bias = (t.float().contiguous().to(DEV) for t in (hidden, logits, vid, W, bias))
    m = None if mask is None else mask.to(DEV).contiguous().view(torch.uint8)
    g = torch.tensor(up, dtype=torch.float32, device=DEV)
    state_bytes, ws_bytes = lib.vs_pretrain_head_state_bytes(B, T, Fo), lib.vs_pretrain_head_workspace_bytes(B, T, d, Fo)
    assert state_bytes > 0 and ws_bytes > 0
    bands = dict(feats=_Band(B * T * Fo * 4, nan=True), state=_Band(state_bytes), losses=_Band(12, nan=True),
                 d_hidden=_Band(B * T * d * 4, nan=True), d_logits=_Band(B * T * 4, nan=True),
                 d_vt_w=_Band(Fo * d * 4, nan=True), d_vt_b=_Band(Fo * 4, nan=True), workspace=_Band(ws_bytes))
    stream = torch.cuda.current_stream().cuda_stream
    mp = None if m is None else m.data_ptr()
    rc = lib.vs_pretrain_head_forward(hidden.data_ptr(), logits.data_ptr(), mp, vid.data_ptr(), W.data_ptr(), bias.data_ptr(),
                                      B, T, d, Fo, temp, int(entropy), bands["feats"].ptr(), bands["state"].ptr(),
                                      bands["losses"].ptr(), stream)
    torch.cuda.synchronize()
    assert rc == L.VS_OK, (rc, lib.vs_last_error())
    rc = lib.vs_pretrain_head_backward(hidden.data_ptr(), logits.data_ptr(), mp, vid.data_ptr(), W.data_ptr(),
                                       bands["feats"].ptr(), bands["state"].ptr(), g.data_ptr(), B, T, d, Fo, temp, int(entropy),
                                       bands["d_hidden"].ptr(), bands["d_logits"].ptr(), bands["d_vt_w"].ptr(),
                                       bands["d_vt_b"].ptr(), bands["workspace"].ptr(), ws_bytes, stream)
    torch.cuda.synchronize()
    assert rc == L.VS_OK, (rc, lib.vs_last_error())
    for name, band in bands.items():
        assert band.intact(), "%s: bytes outside the buffer changed" % name
    return bands


# ---------------------------------------------------------------------------------------------
# 2. a video with every frame masked
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pen", ["entropy", "norm"])
def test_fully_masked_video_yields_nan_like_the_reference(vsa, pen, gemms):
    """Video 1 fully masked beside a valid video 0.  The reference's softmax over -inf scores is NaN: its distillation loss is
    NaN, its norm penalty is NaN, its entropy penalty (masked_fill(mask, 0.)) and its repelling loss are finite - and a NaN
    loss must not come with a clean update.  (Before head_final wrote NaN for Z = 0 the kernels returned a finite distillation
    loss, log-softmax of a zero pooled row, and sqrtf(0) = 0 for the norm penalty.)"""
    B, T, d, Fo = 2, 70, 64, 256
    inputs, vid = _inputs(270, (B, T), d, Fo, B)
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[0, 61:] = True
    mask[1, :] = True
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    want = head_reference(leaves[0], leaves[1], vid, mask, leaves[2], leaves[3], TEMP, pen)
    sum(u * w for u, w in zip(UP, want)).backward()
    want = [w.item() for w in want]
    assert want[0] != want[0] and (want[1] != want[1]) == (pen == "norm") and want[2] == want[2]      # the premise
    bands = _c_padded_head(vsa, inputs[0], inputs[1], mask, vid, inputs[2], inputs[3], TEMP, pen == "entropy")
    got = bands["losses"].floats().cpu().tolist()
    print("fully masked (%s): got %r, float64 %r" % (pen, got, want))
    assert got[0] != got[0], got
    if pen == "norm":
        assert got[1] != got[1], got
    else:
        assert abs(got[1] - want[1]) < 2e-6 * max(1.0, abs(want[1])), (got, want)
    assert abs(got[2] - want[2]) < 2e-6 * max(1.0, abs(want[2])), (got, want)
    assert not torch.isfinite(bands["d_vt_w"].floats()).all() and not torch.isfinite(bands["d_vt_b"].floats()).all()
    assert torch.isnan(bands["d_logits"].floats().view(B, T)[1]).all() and torch.isnan(bands["d_hidden"].floats().view(B, T, d)[1]).all()
    # the valid video beside it keeps its own rows: the reference's are finite, and so are these, at the bars
    for name, n, r in (("d_hidden", d, leaves[0].grad), ("d_logits", 1, leaves[1].grad)):
        a = bands[name].floats().view(B, T, n)[0].double().cpu()
        assert torch.isfinite(r[0]).all() and torch.isfinite(a).all(), name
        err, scale = (a - r[0]).abs().max().item(), r[0].abs().max().item()
        print("fully masked (%s): video 0 %s err %.3e, max %.3e" % (pen, name, err, scale))
        assert err <= 2e-5 * scale + 1e-9, (name, err, scale)


# ---------------------------------------------------------------------------------------------
# 3. padded and packed are the same arithmetic
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pen", ["entropy", "norm"])
@pytest.mark.parametrize("Fo", [256, 768])
@pytest.mark.parametrize("T", [1, 5, 64, 65, 129])
def test_padded_and_packed_heads_are_bit_identical_on_equal_lengths(vsa, T, Fo, pen, gemms):
    """No mask against lengths = [T] * B with ref_len = T: row positions and M are the same, feats is the same GEMM, every
    later stage is the mirrored code (vs_pretrain_kernels.hip: "the same per-frame arithmetic, lane ownership and summation
    order").  Premise, asserted first: two runs of the padded call are bit-identical."""
    B, d = 3, 64
    inputs, vid = _inputs(T * 11 + Fo, (B, T), d, Fo, B)
    padded, packed = _heads()
    up = torch.tensor(UP, device=DEV)

    def run(pk):
        dl = [t.float().to(DEV) for t in inputs]
        if pk:
            dl[0], dl[1] = dl[0].reshape(B * T, d), dl[1].reshape(B * T, 1)
        dl = [t.requires_grad_(True) for t in dl]
        if pk:
            losses = packed.apply(dl[0], dl[1], vid.float().to(DEV), [T] * B, T, dl[2], dl[3], TEMP, pen == "entropy")
        else:
            losses = padded.apply(dl[0], dl[1], vid.float().to(DEV), None, dl[2], dl[3], TEMP, pen == "entropy")
        grads = torch.autograd.grad(losses, dl, grad_outputs=up)
        torch.cuda.synchronize()
        return [losses.detach()] + [g.reshape(-1) for g in grads]

    first, again, mirror = run(False), run(False), run(True)
    assert all(torch.isfinite(t).all() for t in first) and first[1].abs().max().item() > 0
    for a, b, name in zip(first, again, ("losses",) + GRADS):
        assert torch.equal(a, b), "padded, run to run: %s" % name
    for a, b, name in zip(first, mirror, ("losses",) + GRADS):
        assert torch.equal(a, b), "padded against packed: %s, max diff %.3e" % (name, (a - b).abs().max().item())


# ---------------------------------------------------------------------------------------------
# 4. the packed head beyond 64 videos
# ---------------------------------------------------------------------------------------------
CYCLE = (1, 64, 65, 2, 63, 129)      # row and chunk prefix sums that differ from lane to lane, at lanes 63 / 64 of both scan steps


def _lengths(B):
    return [CYCLE[i % len(CYCLE)] for i in range(B)]


def _kid(c):
    B, d, Fo, pen, extra = c
    return "B%d-d%d-F%d-%s%s" % (B, d, Fo, pen, "-ref+%d" % extra if extra else "")


def _packed_want(c):
    if c not in _WANT:
        B, d, Fo, pen, extra = c
        ls = _lengths(B)
        inputs, vid = _inputs(B * 5 + Fo, (sum(ls),), d, Fo, B)
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        want = head_reference_packed(leaves[0], leaves[1], vid, ls, leaves[2], leaves[3], TEMP, pen, max(ls) + extra)
        sum(u * w for u, w in zip(UP, want)).backward()
        _WANT[c] = (inputs, vid, [w.item() for w in want], [t.grad for t in leaves])
    return _WANT[c]


MANY_CASES = [(B, 128, Fo, pen, 0) for B in (64, 65, 128, 129, 130) for Fo in (256, 768) for pen in ("entropy", "norm")]
MANY_CASES += [(130, 128, 256, "entropy", 37)]


@gpu
@pytest.mark.parametrize("case", MANY_CASES, ids=_kid)
def test_packed_head_beyond_64_videos(vsa, case, gemms):
    """pk_locate scans the device lengths 64 per step and carries rows / chunks into the next step: B = 64 ends on the last
    lane of the first step, 65 and 128..130 take the carry once and twice."""
    B, d, Fo, pen, extra = case
    ls = _lengths(B)
    inputs, vid, want_losses, want_grads = _packed_want(case)
    dl = [t.float().to(DEV).requires_grad_(True) for t in inputs]
    got = _heads()[1].apply(dl[0], dl[1], vid.float().to(DEV), ls, max(ls) + extra, dl[2], dl[3], TEMP, pen == "entropy")
    sum(u * g for u, g in zip(UP, got)).backward()
    torch.cuda.synchronize()
    _check(_kid(case), got.detach().cpu(), [t.grad for t in dl], want_losses, want_grads)


@gpu
@pytest.mark.parametrize("pen", ["entropy", "norm"])
def test_videos_across_the_scan_step_do_not_depend_on_their_batch(vsa, pen, gemms):
    """ref_len pinned at 129: videos 63, 64 and 65 of a 130-video batch against the same video packed alone.  d_losses is
    (130, 65, 130) for the batch and (1, 0.5, 1) alone, so the batch-mean factors g0 / (B F), g1 / B and 2 g2 / (B ref_len^2)
    are quotients of the same real numbers - correctly rounded divisions, equal bits - and the rows are bit-equal unscaled."""
    B, d, Fo, ref_len = 130, 128, 256, 129
    ls = _lengths(B)
    inputs, vid = _inputs(130129, (sum(ls),), d, Fo, B)
    hidden, logits, W, bias = (t.float().to(DEV) for t in inputs)
    vid = vid.float().to(DEV)

    def run(h, s, v, lengths, scale):
        h, s = h.clone().requires_grad_(True), s.clone().requires_grad_(True)
        losses = _heads()[1].apply(h, s, v, lengths, ref_len, W, bias, TEMP, pen == "entropy")
        up = torch.tensor([scale * u for u in UP], device=DEV)
        return torch.autograd.grad(losses, [h, s], grad_outputs=up)

    dh, ds = run(hidden, logits, vid, ls, float(B))
    for i in (63, 64, 65):
        r0, r1 = sum(ls[:i]), sum(ls[:i + 1])
        dh1, ds1 = run(hidden[r0:r1], logits[r0:r1], vid[i:i + 1], [ls[i]], 1.0)
        torch.cuda.synchronize()
        assert dh1.abs().max().item() > 0 and (ls[i] == 1 or ds1.abs().max().item() > 0)
        assert torch.equal(ds1, ds[r0:r1]), (pen, i, (ds1 - ds[r0:r1]).abs().max().item())
        assert torch.equal(dh1, dh[r0:r1]), (pen, i, (dh1 - dh[r0:r1]).abs().max().item())


@gpu
@pytest.mark.parametrize("dev_length", [1000, 1])
def test_wrong_device_lengths_at_70_videos_stay_inside_the_buffers(vsa, dev_length, gemms):
    """The contract of include/vs_train.h past the first scan step: a device length is cut at max(lengths), rows beyond Mtot
    and chunks beyond the host's count are cut.  Every buffer the calls write lies between guard bands; both calls return
    VS_OK, the bands are intact and the device goes on working."""
    lib, L = vsa._lib.load(), vsa._lib
    B, d, Fo = 70, 128, 512
    ls = _lengths(B)
    M = sum(ls)
    host = (C.c_int32 * B)(*ls)
    inputs, vid = _inputs(70, (M,), d, Fo, B)
    hidden, logits, W, bias = (t.float().to(DEV) for t in inputs)
    vid = vid.float().to(DEV)
    dlen = torch.full((B,), dev_length, dtype=torch.int32, device=DEV)
    up = torch.tensor(UP, device=DEV)
    state_bytes, ws_bytes = lib.vs_pretrain_head_state_bytes_packed(host, B, Fo), lib.vs_pretrain_head_workspace_bytes_packed(host, B, d, Fo)
    assert state_bytes > 0 and ws_bytes > 0
    bands = dict(feats=_Band(M * Fo * 4), state=_Band(state_bytes), losses=_Band(12), d_hidden=_Band(M * d * 4),
                 d_logits=_Band(M * 4), d_vt_w=_Band(Fo * d * 4), d_vt_b=_Band(Fo * 4), workspace=_Band(ws_bytes))
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.vs_pretrain_head_forward_packed(hidden.data_ptr(), logits.data_ptr(), host, dlen.data_ptr(), B, max(ls), vid.data_ptr(),
                                             W.data_ptr(), bias.data_ptr(), d, Fo, TEMP, 1, bands["feats"].ptr(),
                                             bands["state"].ptr(), bands["losses"].ptr(), stream)
    torch.cuda.synchronize()
    assert rc == L.VS_OK, (rc, lib.vs_last_error())
    rc = lib.vs_pretrain_head_backward_packed(hidden.data_ptr(), logits.data_ptr(), host, dlen.data_ptr(), B, max(ls), vid.data_ptr(),
                                              W.data_ptr(), bands["feats"].ptr(), bands["state"].ptr(), up.data_ptr(), d, Fo, TEMP, 1,
                                              bands["d_hidden"].ptr(), bands["d_logits"].ptr(), bands["d_vt_w"].ptr(),
                                              bands["d_vt_b"].ptr(), bands["workspace"].ptr(), ws_bytes, stream)
    torch.cuda.synchronize()
    assert rc == L.VS_OK, (rc, lib.vs_last_error())
    for name, band in bands.items():
        assert band.intact(), "%s: bytes outside the buffer changed" % name
    assert torch.arange(64, device=DEV).sum().item() == 2016


# ---------------------------------------------------------------------------------------------
# 5. guard bands round the padded head, and its refusals
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masked"])
@pytest.mark.parametrize("B,T,d,Fo", [(3, 65, 64, 768), (1, 1, 32, 1024)])
def test_padded_head_writes_all_of_its_outputs_and_nothing_else(vsa, B, T, d, Fo, masked, gemms):
    """Outputs start as NaN: every element of feats, losses, d_hidden, d_logits, d_vt_w and d_vt_b is overwritten (masked
    rows with their zeros), nothing outside them, head_state or the workspace is touched."""
    inputs, vid = _inputs(B * T + Fo, (B, T), d, Fo, B)
    mask = None
    if masked:      # one video with one frame keeps it: the mask is passed and masks nothing
        mask = _mask(vsa, B, T, "interior") if B > 1 else torch.zeros(B, T, dtype=torch.bool)
    for pen in ("entropy", "norm"):
        bands = _c_padded_head(vsa, inputs[0], inputs[1], mask, vid, inputs[2], inputs[3], TEMP, pen == "entropy")
        for name in ("feats", "losses", "d_hidden", "d_logits", "d_vt_w", "d_vt_b"):
            assert torch.isfinite(bands[name].floats()).all(), "%s (%s): an element was not written" % (name, pen)
        if masked and B > 1:
            assert torch.count_nonzero(bands["d_logits"].floats().view(B, T)[mask.to(DEV)]).item() == 0
            assert torch.count_nonzero(bands["d_hidden"].floats().view(B, T, d)[mask.to(DEV)]).item() == 0


def test_invalid_padded_head_calls_are_refused_before_any_device_access(vsa):
    """Fake, never-dereferenced pointers: every refusal below happens on the host (include/vs_train.h)."""
    lib, L = vsa._lib.load(), vsa._lib
    p = 0x10000

    def fwd(hidden=p, B=2, T=70, d=64, F=256, temp=0.4, losses=p):
        return lib.vs_pretrain_head_forward(hidden, p, None, p, p, p, B, T, d, F, temp, 1, p, p, losses, None)

    def bwd(hidden=p, B=2, T=70, d=64, F=256, temp=0.4, ws=0x20000, ws_bytes=1 << 40, d_vt_b=p):
        return lib.vs_pretrain_head_backward(hidden, p, None, p, p, p, p, p, B, T, d, F, temp, 1, p, p, p, d_vt_b, ws, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(d=100) == L.VS_ERR_INVALID and b"d=100" in lib.vs_last_error()
        assert call(F=384) == L.VS_ERR_INVALID and b"F=384" in lib.vs_last_error()
        assert call(temp=0.0) == L.VS_ERR_INVALID and b"temp=0" in lib.vs_last_error()
        assert call(B=0) == L.VS_ERR_INVALID and call(T=0) == L.VS_ERR_INVALID
        assert call(hidden=None) == L.VS_ERR_INVALID and b"NULL" in lib.vs_last_error()
    assert fwd(losses=None) == L.VS_ERR_INVALID and b"NULL" in lib.vs_last_error()
    assert bwd(d_vt_b=None) == L.VS_ERR_INVALID and b"NULL" in lib.vs_last_error()
    assert bwd(ws=None) == L.VS_ERR_INVALID and b"NULL" in lib.vs_last_error()
    need = lib.vs_pretrain_head_workspace_bytes(2, 70, 64, 256)
    assert need >= 2 * 70 * 256 * 4 and need % 256 == 0
    assert bwd(ws_bytes=need - 1) == L.VS_ERR_WORKSPACE and b"workspace" in lib.vs_last_error()
    assert bwd(ws=0x20010, ws_bytes=need) == L.VS_ERR_WORKSPACE          # not 256-byte aligned
    assert lib.vs_pretrain_head_state_bytes(0, 70, 256) == 0 and lib.vs_pretrain_head_workspace_bytes(2, 70, 0, 256) == 0
