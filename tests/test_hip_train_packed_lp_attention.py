"""GPU tests of the OPT-IN 16-bit attention of packed ragged training (VS_TRAIN_FLAG_PACKED_LP_ATTENTION,
SimNet.set_train_dtype(..., packed_attention=True); the packed kernels of csrc/vs_train_attention_bf16.hip).

1. dropout off: every video of a packed batch gets, bit for bit, what the PADDED 16-bit kernels give for that video alone -
   the packed kernels differ from the padded ones only in where a block's rows and keep words live, and this pins the index maps;
2. dropout on, one-video batches: Mtot = T makes the dropout row keys equal, so the packed hooks reproduce the padded hooks
   fed with vs_train_attention_dropout_bits(B = 1), bit for bit;
3. dropout on, many videos: against float64 per video with the library's own keep masks, at the bounds of
   test_hip_train.test_attention_forward_and_backward_kernels_bf16;
4. whole steps on the reference's float64 packed goldens at tests/tolerances.py's TRAIN_LP_* / TRAIN_FP16_*;
5. the default (no keyword) is untouched, before and after a step that used the opt-in;
6. PretrainModel.forward_packed inherits the mode.

The edge batch crosses owner tiles (128), streamed tiles (64) and keep words (32) with odd row offsets from the second video
on.  The CPU part (symbols, argument checks, scratch size, the keyword) is tests/test_train_packed_lp_host.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import torch_ref
import tolerances as tol
import test_hip_pretrain_packed as pre
from test_hip_train_packed import _close, _cu, _dev, _i32, _model, _packed_inputs, _packed_step, _stream, packed_cases

pytestmark = pytest.mark.gpu

LENGTHS = [129, 1, 64, 257, 33, 128, 63, 2, 65, 31, 127, 32]          # 932 rows; one, three and five streamed tiles
SHAPES = [(2, 32), (2, 64), (2, 128)]
F16_BIT = 64                                                         # in16 & 64 of the padded hooks: the 16-bit type is fp16
SEED, SITE = 0x1234567887654321, 7


@pytest.fixture
def lp_train_everywhere(vsa):
    vsa._lib.set_option("VS_TRAIN_LP_MIN_ROWS", 0)
    yield
    vsa._lib.set_option("VS_TRAIN_LP_MIN_ROWS", -1)


def _operands(lengths, H, dh, dtype=torch.float32):
    M, d = sum(lengths), H * dh
    g = torch.Generator().manual_seed(100 + M + dh)
    q, k, v = (torch.randn(H, M, dh, generator=g, dtype=dtype) for _ in range(3))
    dO = torch.randn(M, d, generator=torch.Generator().manual_seed(9), dtype=dtype)
    return q, k, v, dO


def _packed_lp(vsa, q, k, v, dO, lengths, H, dh, scale, p, f16):
    """out [M, d], lse2 [H, M], dqkv [M, 3d] of the packed 16-bit kernels; outputs prefilled with NaN"""
    lib = vsa._lib.load()
    B, M, d = len(lengths), sum(lengths), H * dh
    host, dl = _i32(lengths), torch.tensor(lengths, dtype=torch.int32, device=_dev())
    ws = torch.empty(lib.vs_train_attention_packed_lp_scratch_bytes(host, B, H), dtype=torch.uint8, device=_dev())
    out = torch.full((M, d), float("nan"), device=_dev())
    lse = torch.full((H, M), float("nan"), device=_dev())
    dqkv = torch.full((M, 3 * d), float("nan"), device=_dev())
    vsa._lib.check(lib.vs_train_attention_forward_packed_lp(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), host,
                                                            dl.data_ptr(), B, H, dh, scale, SEED, SITE, p, f16, ws.data_ptr(), ws.numel(),
                                                            _stream()))
    vsa._lib.check(lib.vs_train_attention_backward_packed_lp(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dO.data_ptr(),
                                                             lse.data_ptr(), dqkv.data_ptr(), host, dl.data_ptr(), B, H, dh, scale, SEED, SITE,
                                                             p, f16, ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    return out, lse, dqkv


def _padded_lp_alone(vsa, q, k, v, dO, H, dh, scale, p, f16):
    """one video alone through the PADDED 16-bit kernels (B = 1, T = its length, no mask, fp32-stored operands): q, k, v [H, T, dh],
    dO [T, d] -> out [T, d], lse2 [H, T], dqkv [T, 3d]; p > 0: the keep words of vs_train_attention_dropout_bits(B = 1)"""
    lib = vsa._lib.load()
    T, d = q.shape[1], H * dh
    q, k, v, dO = (t.contiguous() for t in (q, k, v, dO))
    dbits = None
    if p > 0:
        dbits = torch.empty(lib.vs_train_attention_dropout_bits_bytes(1, H, T), dtype=torch.uint8, device=_dev())
        vsa._lib.check(lib.vs_train_attention_dropout_bits(dbits.data_ptr(), 1, H, T, SEED, SITE, p, _stream()))
    dp = None if dbits is None else dbits.data_ptr()
    in16 = F16_BIT if f16 else 0
    out = torch.full((T, d), float("nan"), device=_dev())
    lse = torch.full((H, T), float("nan"), device=_dev())
    dqkv = torch.full((T, 3 * d), float("nan"), device=_dev())
    scratch = torch.empty(H * T, device=_dev())
    vsa._lib.check(lib.vs_train_attention_forward_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, out.data_ptr(), lse.data_ptr(), 1, H, T, dh,
                                                       scale, p, dp, in16, _stream()))
    vsa._lib.check(lib.vs_train_attention_backward_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, out.data_ptr(), dO.data_ptr(), lse.data_ptr(),
                                                        dqkv.data_ptr(), scratch.data_ptr(), 1, H, T, dh, scale, p, dp, in16, _stream()))
    torch.cuda.synchronize()
    return out, lse, dqkv


# ---------------------------------------------------------------------------------------------
# 1. bit identity with the padded kernel, dropout off
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,dh", SHAPES)
def test_every_video_gets_the_bits_of_the_padded_kernel_running_it_alone(vsa, H, dh, f16):
    """p = 0: out[sl], lse2[:, sl], dqkv[sl] of every video of LENGTHS are torch.equal to vs_train_attention_forward_bf16 /
    _backward_bf16 on that video alone.  Every output row is written (NaN prefill), and a second run gives the same bits."""
    lengths, cu = LENGTHS, _cu(LENGTHS)
    scale = (H * dh) ** -0.5
    q, k, v, dO = (t.to(_dev()) for t in _operands(lengths, H, dh))
    out, lse, dqkv = _packed_lp(vsa, q, k, v, dO, lengths, H, dh, scale, 0.0, f16)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    again = _packed_lp(vsa, q, k, v, dO, lengths, H, dh, scale, 0.0, f16)
    assert all(torch.equal(a, b) for a, b in zip((out, lse, dqkv), again))
    for b, t in enumerate(lengths):
        sl = slice(cu[b], cu[b + 1])
        o1, l1, g1 = _padded_lp_alone(vsa, q[:, sl], k[:, sl], v[:, sl], dO[sl], H, dh, scale, 0.0, f16)
        assert torch.isfinite(o1).all() and torch.isfinite(l1).all() and torch.isfinite(g1).all(), (b, t)
        assert torch.equal(out[sl], o1), ("out", b, t)
        assert torch.equal(lse[:, sl], l1), ("lse2", b, t)
        assert torch.equal(dqkv[sl], g1), ("dqkv", b, t)


# ---------------------------------------------------------------------------------------------
# 2. bit identity with dropout, one-video batches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
@pytest.mark.parametrize("T", [129, 65])
@pytest.mark.parametrize("H,dh", SHAPES)
def test_a_one_video_batch_with_dropout_is_the_padded_call(vsa, H, dh, T, f16):
    """p = 0.3, lengths [T]: with Mtot = T the dropout row key head * Mtot + row equals the padded bh * T + row, so the packed
    keep words are those of vs_train_attention_dropout_bits(B = 1) and the outputs the padded hooks' bits."""
    scale, p = (H * dh) ** -0.5, 0.3
    q, k, v, dO = (t.to(_dev()) for t in _operands([T], H, dh))
    got = _packed_lp(vsa, q, k, v, dO, [T], H, dh, scale, p, f16)
    want = _padded_lp_alone(vsa, q, k, v, dO, H, dh, scale, p, f16)
    for name, a, b in zip(("out", "lse2", "dqkv"), got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    off = _packed_lp(vsa, q, k, v, dO, [T], H, dh, scale, 0.0, f16)
    assert not torch.equal(off[0], got[0]), "dropout did not reach the kernels"


# ---------------------------------------------------------------------------------------------
# 3. many videos with dropout, against float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,dh,f16", [(2, 32, 0), (2, 64, 0), (2, 128, 0), (2, 64, 1)], ids=["h2-dh32-bf16", "h2-dh64-bf16", "h2-dh128-bf16", "h2-dh64-fp16"])
def test_packed_lp_attention_against_float64_with_the_librarys_keep_masks(vsa, H, dh, f16):
    """the checker of test_hip_train_packed_edges.test_packed_attention_kernels_at_tile_and_keep_word_edges (float64 per video,
    the keep mask of vs_train_dropout_mask_attention_packed) at the bounds of
    test_hip_train.test_attention_forward_and_backward_kernels_bf16: out 1.5e-2 of the tensor's largest entry, lse2 2e-2, dq /
    dk / dv 3e-2, and that test's 3e-3 floor on dq / dk of the one-frame video (fp16 is tighter than bf16: same bounds)."""
    lib = vsa._lib.load()
    lengths, cu, p = LENGTHS, _cu(LENGTHS), 0.3
    B, d = len(lengths), H * dh
    scale = d ** -0.5
    q, k, v, dO = _operands(lengths, H, dh, torch.float64)
    kd = torch.empty(H * sum(t * t for t in lengths), dtype=torch.uint8, device=_dev())
    vsa._lib.check(lib.vs_train_dropout_mask_attention_packed(kd.data_ptr(), _i32(lengths), B, H, SEED, SITE, p, _stream()))
    kd, off, keep = kd.cpu(), 0, []
    for t in lengths:
        keep.append(kd[off: off + H * t * t].view(1, H, t, t))
        off += H * t * t
    rate = kd.double().mean().item()
    assert abs(rate - (1 - p)) < 5 * math.sqrt(p * (1 - p) / kd.numel()), rate
    qd, kd_, vd, dOd = (t.float().to(_dev()).contiguous() for t in (q, k, v, dO))
    out, lse, dqkv = _packed_lp(vsa, qd, kd_, vd, dOd, lengths, H, dh, scale, p, f16)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()       # every row written
    worst = {}
    for b, t in enumerate(lengths):
        sl = slice(cu[b], cu[b + 1])
        qb, kb, vb = (u[:, sl][None].clone().requires_grad_(True) for u in (q, k, v))
        want, lse2 = torch_ref.attention_with_mask(qb, kb, vb, None, scale, keep[b], p)
        want.backward(dO[sl][None])
        worst["out"] = max(worst.get("out", 0.0), _close(out[sl], want[0], "attention out, video %d" % b, atol=None, rtol=1.5e-2))
        lerr = (lse[:, sl].cpu().double() - lse2.detach()[0]).abs().max().item()
        worst["lse2"] = max(worst.get("lse2", 0.0), lerr)
        assert lerr < 2e-2, (b, lerr)
        tok = lambda gr: gr[0].permute(1, 0, 2).reshape(t, d)       # noqa: E731  head-major grad -> token-major
        floor = 3e-3 if t == 1 else 0.0
        for name, got, ref in (("dq", dqkv[sl, :d], tok(qb.grad)), ("dk", dqkv[sl, d:2 * d], tok(kb.grad))):
            if floor and ref.abs().max().item() < floor:
                assert got.abs().max().item() < floor, (name, b)
            else:
                worst[name] = max(worst.get(name, 0.0), _close(got, ref, "%s, video %d" % (name, b), atol=None, rtol=3e-2))
        worst["dv"] = max(worst.get("dv", 0.0), _close(dqkv[sl, 2 * d:], tok(vb.grad), "dv, video %d" % b, atol=None, rtol=3e-2))
    print("packed %s attention, H %d dh %d, worst error relative to a video's largest entry (lse2: absolute): %s"
          % ("fp16" if f16 else "bf16", H, dh, {n: "%.2e" % e for n, e in worst.items()}))


# ---------------------------------------------------------------------------------------------
# 4. whole steps on the reference's float64 goldens
# ---------------------------------------------------------------------------------------------
def _check_low_precision_step(z, loss, grads, name):
    """the assertions of test_hip_train_packed.test_packed_bf16_training_gradients_within_the_low_precision_tolerance, with its fc1
    ReLU-flip allowance"""
    want = float(z["loss"])
    assert abs(loss.item() - want) <= tol.TRAIN_LP_LOSS_RTOL * max(1.0, abs(want)), (loss.item(), want)
    worst, worst_l2 = 0.0, 0.0
    for k in json.loads(str(z["keys"])):
        g = grads[k]
        assert g is not None and torch.isfinite(g).all(), k
        g2 = g.reshape(-1, g.shape[-1]) if g.dim() > 1 else g.reshape(1, -1)
        rows = torch.from_numpy(z["r:" + k])
        want_g = torch.from_numpy(z["g:" + k]).double()
        tot, nrm, gmax, ref32 = z["s:" + k]
        diff = g2[rows.to(g2.device)].double().cpu() - want_g
        err = diff.abs().max().item()
        l2 = diff.norm().item() / (want_g.norm().item() + 1e-30)
        if gmax < 1e-6:
            assert g.double().norm().item() <= tol.TRAIN_LP_ZERO_ATOL, "%s: |g| %.3e" % (k, g.double().norm().item())
            continue
        assert err <= tol.TRAIN_LP_GRAD_RTOL * gmax + 1e-6, "%s: err %.3e, max|g| %.3e" % (k, err, gmax)
        if k.endswith("mlp.fc1.weight") and diff.dim() > 1 and diff.shape[0] >= 4 and l2 > tol.TRAIN_LP_GRAD_L2:
            sq = diff.pow(2).sum(-1)                         # the ReLU-flip allowance of tests/tolerances.py, fc1.weight only
            keep_rows = torch.ones_like(sq, dtype=torch.bool)
            keep_rows[sq.argmax()] = False
            l2 = sq[keep_rows].sum().sqrt().item() / (want_g[keep_rows].norm().item() + 1e-30)
            assert l2 <= tol.TRAIN_LP_FC1_L2, "%s: relative L2 error %.3e with the flipped unit's row set aside" % (k, l2)
            l2 = 0.0
        assert l2 <= (tol.TRAIN_LP_FC1_L2 if k.endswith("mlp.fc1.bias") else tol.TRAIN_LP_GRAD_L2), "%s: relative L2 error %.3e" % (k, l2)
        assert abs(g.double().norm().item() - nrm) <= 2e-2 * nrm + 1e-7, k
        worst, worst_l2 = max(worst, err / gmax), max(worst_l2, l2)
    assert worst > 1e-5, "the low-precision path did not run (gradients at exact-fp32 accuracy)"
    print("%s: bf16 Linears + packed bf16 attention, worst error relative to the tensor's max %.2e, worst relative L2 %.2e" % (name, worst, worst_l2))


@pytest.mark.parametrize("name", ["train_packed_ma", "train_packed_mb"])          # head dim 64 and 128 (tests/golden/train_packed_index.json)
def test_packed_lp_attention_training_gradients_within_the_low_precision_tolerance(vsa, lp_train_everywhere, name):
    c = [k for k in packed_cases() if k["name"] == name][0]
    assert c["d"] // c["H"] in (32, 64, 128)
    z = np.load(os.path.join(GOLDEN, c["name"] + ".npz"))
    xp, tp, R, lengths = _packed_inputs(vsa, c)
    fmt = lambda: int(vsa._lib.load().vs_train_last_format())      # noqa: E731
    m = _model(vsa, c).set_train_dtype("bf16")
    _, _, plain = _packed_step(vsa, m, c, xp, tp, R, lengths)
    assert (fmt() & 3) == 1 and m.last_packed_attention_dtype == "fp32"
    plain = {k: g.clone() for k, g in plain.items()}
    m.set_train_dtype("bf16", packed_attention=True)
    m.zero_grad(set_to_none=True)
    loss, pred, grads = _packed_step(vsa, m, c, xp, tp, R, lengths)
    assert (fmt() & 3) == 3 and (fmt() & 4) == 0          # 16-bit Linears and attention; q / k / v of the record stay fp32
    assert m.last_train_dtype == "bf16" and m.last_packed_attention_dtype == "bf16"
    _check_low_precision_step(z, loss, grads, name)
    assert any(not torch.equal(grads[k], plain[k]) for k in grads), "the packed 16-bit attention did not run"
    m.set_train_dtype("fp16", packed_attention=True)
    m.zero_grad(set_to_none=True)
    loss16, _, g16 = _packed_step(vsa, m, c, xp, tp, R, lengths)
    want = float(z["loss"])
    assert (fmt() & 35) == 35 and m.last_train_dtype == "fp16" and m.last_packed_attention_dtype == "fp16"
    assert abs(loss16.item() - want) <= tol.TRAIN_FP16_LOSS_RTOL * max(1.0, abs(want)), (loss16.item(), want)
    assert all(torch.isfinite(t).all() for t in g16.values())


# ---------------------------------------------------------------------------------------------
# 5. the default is untouched
# ---------------------------------------------------------------------------------------------
def test_the_default_is_bit_identical_before_and_after_an_opt_in_step(vsa, lp_train_everywhere):
    """set_train_dtype("bf16") without the keyword: format & 3 == 1 (exact packed attention), and two such steps with one seed
    are bit-equal around a step that used the opt-in - nothing of the mode stays behind in the module or the library."""
    c = dict(H=4, d=256, L=2, wseed=5, hidden_w=1e-3)
    lengths = [129, 65, 33, 2]
    M = sum(lengths)
    x = torch.randn(M, 1024, generator=torch.Generator().manual_seed(2))
    target = torch.rand(M, generator=torch.Generator().manual_seed(3))
    R = torch.randn(M, c["d"], generator=torch.Generator().manual_seed(4))
    m = _model(vsa, c, dropout=0.3)
    fmt = lambda: int(vsa._lib.load().vs_train_last_format())      # noqa: E731

    def step(**kw):
        m.set_train_dtype("bf16", **kw)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        loss, pred, grads = _packed_step(vsa, m, c, x, target, R, lengths)
        return fmt(), [loss.detach().clone(), pred.detach().clone()] + [grads[k].clone() for k in sorted(grads)]
    f0, before = step()
    f1, opted = step(packed_attention=True)
    f2, after = step()
    assert (f0 & 3) == 1 and (f1 & 3) == 3 and (f2 & 3) == 1 and f0 == f2
    assert m.last_packed_attention_dtype == "fp32"
    assert all(torch.isfinite(a).all() and torch.equal(a, b) for a, b in zip(before, after))
    assert any(not torch.equal(a, b) for a, b in zip(before, opted))


# ---------------------------------------------------------------------------------------------
# 6. pretraining
# ---------------------------------------------------------------------------------------------
def test_pretrain_forward_packed_inherits_the_mode(vsa, lp_train_everywhere):
    """PretrainModel.forward_packed + backward on pretrain_packed_ma with the opt-in on its encoder: the three losses within
    TRAIN_LP_LOSS_RTOL of the golden's, every gradient finite, the format word reports the packed 16-bit attention (the loss
    head stays exact fp32)."""
    c = [k for k in pre.golden_cases() if k["name"] == "pretrain_packed_ma"][0]
    assert c["d"] // c["H"] in (32, 64, 128)
    z = np.load(os.path.join(GOLDEN, c["name"] + ".npz"))
    m = pre._golden_model(vsa, c)
    m.encoder.set_train_dtype("bf16", packed_attention=True)
    losses, grads = pre._packed_step(m, c, *pre._golden_inputs(vsa, c))
    assert (int(vsa._lib.load().vs_train_last_format()) & 3) == 3
    assert m.encoder.last_train_dtype == "bf16" and m.encoder.last_packed_attention_dtype == "bf16"
    for got, want in zip(losses.tolist(), z["losses"].tolist()):
        print("bf16 encoder + packed bf16 attention: loss %.9f (float64 %.9f)" % (got, want))
        assert abs(got - want) <= tol.TRAIN_LP_LOSS_RTOL * max(1.0, abs(want)), (got, want)
    assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
