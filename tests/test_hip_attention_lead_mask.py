"""GPU: every attention kernel on key masks whose LEADING keys are dead (tests/lead_mask_cases.py), against float64.

Each kernel guards "this row has seen no live key yet" (running maximum -inf) by hand; no other deterministic test reaches that
state from a key mask.  The batch dimension carries the position of the first live key, so one launch per (kernel, head dim, T)
covers every position; both mask families run (lead: keys < f dead; mixed: holes and dead tails behind key f as well).

No tolerance is new: each kernel is held to the bound its own test in test_hip_parity.py / test_hip_attention_maps.py /
test_hip_train.py states, on unit-gain inputs (tests/test_lead_mask_cases_host.py shows a plain fp32 restatement 4x inside the
exact ones).  Every case prints its worst error / bound ratio before it asserts.  On top of "close": outputs are finite, dead
keys get exactly zero map columns and exactly zero dk / dv rows, the video whose only live key is T - 1 is reproduced bit for
bit by the exact kernels, and (where the kernel promises it) a video scored alone gives the bits it had in the batch."""
import math

import numpy as np
import pytest
import torch

import attn_cases
import lead_mask_cases as lm
import tolerances as tol
from oracle.simnet_oracle import oracle_forward
from test_hip_parity import (BF16_STORED_REL, _attn_ref_bf16_operands, _attn_ref_stored, _run_attn_stored, _stored_operands)
from test_hip_train import _close

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-5                      # test_attention_kernel, test_attention_f16x3_kernel
LSE_TOL = 1e-4                      # test_attention_forward_and_backward_kernels
LP_OUT, LP_LSE, LP_GRAD = 1.5e-2, 2e-2, 3e-2      # test_attention_forward_and_backward_kernels_bf16
SEED, SITE = 0x1234567887654321, 7
LOG2E = 1.4426950408889634
H = 2

both_families = pytest.mark.parametrize("family", lm.FAMILIES)


def _grid(dhs, Ts):
    return [(dh, T) for dh in dhs for T in Ts]


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _report(kernel, dh, T, family, **ratios):
    """the line DESIGN.md's table is read from: every figure is an error divided by the bound it is held to"""
    print("lead-mask %-28s dh %3d T %3d %-5s worst err/bound %.3f  (%s)"
          % (kernel, dh, T, family, max(ratios.values()), " ".join("%s %.3f" % kv for kv in ratios.items())))


def _device_case(T, dh, family):
    q, k, v, scale, dO = lm.case_inputs(T, dh)
    mask = lm.mask(T, family)
    dev = _dev()
    return (q.to(dev), k.to(dev), v.to(dev), mask.to(dev).view(torch.uint8), dO.to(dev)), (q, k, v, mask, scale, dO)


def _scoring(vsa, entry, q, k, v, m, scale):
    """vs_attention_f32 / _f16x3 / _bf16 on device tensors; out [B, T, H * dh], prefilled with NaN"""
    B, Hh, T, dh = q.shape
    out = torch.full((B, T, Hh * dh), float("nan"), device=q.device)
    vsa._lib.check(getattr(vsa._lib.load(), entry)(q.data_ptr(), k.data_ptr(), v.data_ptr(), _ptr(m), out.data_ptr(), B, Hh, T, dh, scale,
                                                   _stream()))
    torch.cuda.synchronize()
    return out


def _alone(t, b):
    return t[b:b + 1].contiguous()


def _one_hot_rows(v, T):
    """what the video whose only live key is T - 1 must return in every row: V[b, h, T - 1, :], token-major"""
    b = lm.only_last_live(T)
    return b, v[b, :, T - 1, :].reshape(1, -1).expand(T, -1)


# ---- scoring kernels -------------------------------------------------------------------------------------------------
@both_families
@pytest.mark.parametrize("dh,T", _grid((32, 64), lm.LENGTHS) + _grid((128,), (65, 200)))
def test_attention_f32(vsa, dh, T, family):
    """attn_fwd_pipe in 4- and 8-wave blocks and attn_fwd<128, 1>.  The one-hot video is exact: the first live block's fix-up
    sets the row constant to that block's maximum, the one live score, so p = exp2(0) = 1, l = 1 and every other term of the
    output is 0 * finite."""
    (q, k, v, m, _), (_, _, vh, _, scale, _) = _device_case(T, dh, family)
    ref = lm.reference64(T, dh, family)[0]
    out = _scoring(vsa, "vs_attention_f32", q, k, v, m, scale)
    err = (out.cpu().double() - ref).abs().max().item()
    _report("vs_attention_f32", dh, T, family, out=err / OUT_TOL)
    assert torch.isfinite(out).all()
    assert err < OUT_TOL, err
    for b in range(q.shape[0]):
        one = _scoring(vsa, "vs_attention_f32", _alone(q, b), _alone(k, b), _alone(v, b), _alone(m, b), scale)
        assert torch.equal(one[0], out[b]), ("alone", b, lm.first_live(T)[b])
    if family == "lead":
        b, want = _one_hot_rows(vh, T)
        assert torch.equal(out[b].cpu(), want), (out[b].cpu() - want).abs().max().item()


@both_families
@pytest.mark.parametrize("dh,T", _grid((32, 64), (65, 200, 320)))
def test_attention_f16x3(vsa, dh, T, family):
    (q, k, v, m, _), (*_, scale, _) = _device_case(T, dh, family)
    ref = lm.reference64(T, dh, family)[0]
    out = _scoring(vsa, "vs_attention_f16x3", q, k, v, m, scale)
    err = (out.cpu().double() - ref).abs().max().item()
    _report("vs_attention_f16x3", dh, T, family, out=err / OUT_TOL)
    assert torch.isfinite(out).all()
    assert err < OUT_TOL, err


@both_families
@pytest.mark.parametrize("dh,T", _grid((32, 64, 128), (65, 200, 320)))
def test_attention_bf16(vsa, dh, T, family):
    (q, k, v, m, _), (qh, kh, vh, mask, scale, _) = _device_case(T, dh, family)
    ref = lm.reference64(T, dh, family)[0]
    ref_b = _attn_ref_bf16_operands(qh, kh, vh, mask, scale)
    out = _scoring(vsa, "vs_attention_bf16", q, k, v, m, scale).cpu()
    e_ref = (out.double() - ref).abs().max().item() / ref.abs().max().item()
    e_shared = (out.double() - ref_b).abs().max().item() / ref_b.abs().max().item()
    _report("vs_attention_bf16", dh, T, family, float64=e_ref / tol.BF16_ATTN_KERNEL_REL, shared_rounding=e_shared / 4e-3)
    assert torch.isfinite(out).all()
    assert e_ref < tol.BF16_ATTN_KERNEL_REL and e_shared < 4e-3, (e_ref, e_shared)


@both_families
@pytest.mark.parametrize("T", lm.LENGTHS)
def test_attention_bf16_stored_head_dim_64(vsa, T, family):
    """The one-wave-per-SIMD kernel in both passes (optimistic first / every tile checked) and the 8-wave attn_fwd_lp_pipe, as
    in test_attention_bf16_stored_w64_kernel; each of the three gives a video scored alone the bits it had in the batch."""
    qh, kh, vh, scale, _ = lm.case_inputs(T, 64)
    mask = lm.mask(T, family)
    q16, k16, v16 = _stored_operands(qh, kh, vh, scale)
    ref = _attn_ref_stored(q16, k16, v16, mask)
    big = ref.abs().max().item()
    outs = {cfg: _run_attn_stored(vsa, q16, k16, v16, mask, *cfg) for cfg in ((1, 0), (1, 1), (0, 0))}
    err = {cfg: (o.double() - ref).abs().max().item() / big for cfg, o in outs.items()}
    gap = {cfg: (outs[cfg].double() - outs[(0, 0)].double()).abs().max().item() / big for cfg in ((1, 0), (1, 1))}
    _report("vs_attention_bf16_stored", 64, T, family, w64=err[(1, 0)] / BF16_STORED_REL, w64_checked=err[(1, 1)] / BF16_STORED_REL,
            lp_pipe=err[(0, 0)] / BF16_STORED_REL, w64_vs_lp_pipe=max(gap.values()) / (2 * BF16_STORED_REL))
    assert all(torch.isfinite(o).all() for o in outs.values())
    assert all(e < BF16_STORED_REL for e in err.values()), err
    assert all(g < 2 * BF16_STORED_REL for g in gap.values()), gap
    for cfg, o in outs.items():
        for b in range(q16.shape[0]):
            one = _run_attn_stored(vsa, _alone(q16, b), _alone(k16, b), _alone(v16, b), _alone(mask, b), *cfg)
            assert torch.equal(one[0], o[b]), ("alone", cfg, b, lm.first_live(T)[b])


@both_families
@pytest.mark.parametrize("dh", [32, 128])
def test_attention_bf16_stored_other_head_dims(vsa, dh, family):
    T = 200
    qh, kh, vh, scale, _ = lm.case_inputs(T, dh)
    mask = lm.mask(T, family)
    q16, k16, v16 = _stored_operands(qh, kh, vh, scale)
    ref = _attn_ref_stored(q16, k16, v16, mask)
    out = _run_attn_stored(vsa, q16, k16, v16, mask)
    err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
    _report("vs_attention_bf16_stored", dh, T, family, lp_pipe=err / BF16_STORED_REL)
    assert torch.isfinite(out).all()
    assert err < BF16_STORED_REL, err


# ---- the maps kernel ---------------------------------------------------------------------------------------------------
@both_families
@pytest.mark.parametrize("dh,T", _grid((32, 64, 128, 256), (65, 200, 320)))
def test_attention_probs(vsa, dh, T, family):
    """maps, received and entropy against attn_cases.reductions64 of the float64 maps.  The one-hot video: the row constant is
    m + log2(l) with l = exp2(0) = 1, the entropy sum has one term 1 * 0 (dead keys add 0, not 0 * -inf), and the apply pass
    arrives at the same bits for s when it forms exp2(s - c), so the map row is exactly one-hot and its entropy exactly 0."""
    lib = vsa._lib.load()
    (q, k, _, m, _), (_, _, _, mask, scale, _) = _device_case(T, dh, family)
    B = q.shape[0]
    P = lm.reference64(T, dh, family)[2].numpy()
    dead = mask.numpy()
    rec64, ent64 = attn_cases.reductions64(P, ~dead)
    maps = torch.full((B, H, T, T), float("nan"), device=_dev())
    received = torch.full((B, H, T), float("nan"), device=_dev())
    entropy = torch.full((B, H, T), float("nan"), device=_dev())
    ws = torch.empty((lib.vs_attention_probs_workspace_bytes(B, H, T),), dtype=torch.uint8, device=_dev())
    vsa._lib.check(lib.vs_attention_probs_f32(q.data_ptr(), k.data_ptr(), m.data_ptr(), maps.data_ptr(), received.data_ptr(), entropy.data_ptr(),
                                              B, H, T, dh, scale, ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    maps, received, entropy = maps.cpu().numpy(), received.cpu().numpy(), entropy.cpu().numpy()
    vq = ~dead
    d_map = np.abs(maps - P)[np.broadcast_to(vq[:, None, :, None], P.shape)].max()
    d_ent = np.abs(entropy - ent64)[np.broadcast_to(vq[:, None, :], ent64.shape)].max()
    d_rec = np.abs(received - rec64).max()
    _report("vs_attention_probs_f32", dh, T, family, maps=d_map / tol.FP32_TOL, received=d_rec / tol.FP32_TOL, entropy=d_ent / tol.FP32_TOL)
    assert not np.isnan(maps).any() and not np.isnan(received).any() and not np.isnan(entropy).any()
    assert np.all(maps[np.broadcast_to(dead[:, None, None, :], maps.shape)] == 0.0), "dead key columns must be exactly 0"
    assert max(d_map, d_ent, d_rec) < tol.FP32_TOL, (d_map, d_ent, d_rec)
    if family == "lead":
        b = lm.only_last_live(T)
        one_hot = np.zeros((H, T, T), dtype=np.float32)
        one_hot[:, :, T - 1] = 1.0
        print("one-hot video: map off by %.2e, entropy %.2e" % (np.abs(maps[b] - one_hot).max(), np.abs(entropy[b]).max()))
        assert np.array_equal(maps[b], one_hot)
        assert np.all(entropy[b] == 0.0)


# ---- training kernels ----------------------------------------------------------------------------------------------------
_DROP_REF = {}


def _keep_bytes(vsa, B, T, p):
    keep = torch.empty(B, H, T, T, dtype=torch.uint8, device=_dev())
    vsa._lib.check(vsa._lib.load().vs_train_dropout_mask_attention(keep.data_ptr(), B, H, T, SEED, SITE, p, _stream()))
    torch.cuda.synchronize()
    return keep.cpu()


def _train_reference(vsa, T, dh, family, p):
    """float64 (out, lse2, P, dq, dk, dv); with p > 0 the library's own keep bytes enter torch_ref's dropout formula
    (lead_mask_cases.attention is torch_ref.attention_with_mask that also returns the maps).  Computed once per case."""
    if p == 0.0:
        return lm.reference64(T, dh, family)
    key = (T, dh, family, p)
    if key not in _DROP_REF:
        q, k, v, scale, dO = lm.case_inputs(T, dh)
        keep = _keep_bytes(vsa, q.shape[0], T, p)
        rate = keep.double().mean().item()
        assert abs(rate - (1 - p)) < 4 * math.sqrt(p * (1 - p) / keep.numel()) + 1e-3, rate
        _DROP_REF[key] = lm.attention_grads(q, k, v, lm.mask(T, family), scale, dO, torch.float64, keep, p)
    return _DROP_REF[key]


def _ratio(got, want, atol, rtol):
    """error over the bound _close holds it to: err <= atol (if any) and err <= rtol * max |want| + 1e-6"""
    err = (got.detach().double().cpu() - want).abs().max().item()
    bound = rtol * want.abs().max().item() + 1e-6
    return err / (bound if atol is None else min(atol, bound))


def _assert_dead_keys_get_no_gradient(dqkv, mask, d, what):
    dead = mask[:, :, None].expand(-1, -1, d)
    dk, dv = dqkv[:, :, d:2 * d].cpu(), dqkv[:, :, 2 * d:].cpu()
    assert (dk[dead] == 0.0).all() and (dv[dead] == 0.0).all(), what + ": dk / dv rows of dead keys must be exactly 0.0"


@pytest.mark.parametrize("p", [0.0, 0.3])
@both_families
@pytest.mark.parametrize("dh,T", _grid((32, 64, 128), (65, 200, 320)) + [(256, 65)])
def test_train_attention_exact(vsa, dh, T, family, p):
    """attn_fwd_train / attn_bwd_dq / attn_bwd_dkdv with the hash dropout (DROP == 1) and without.  p = 0: a video run alone gives
    the forward's bits (with dropout the hash is keyed by the row's index in the batch, so only p = 0 can promise that), and the
    one-hot video is exact: m_use is the one live score, p = exp2(0) = 1, l = 1, inv = 1, every other product is 0 * finite."""
    lib = vsa._lib.load()
    (q, k, v, m, dO), (_, _, vh, mask, scale, _) = _device_case(T, dh, family)
    B, d = q.shape[0], H * dh
    want, lse2, _, gq, gk, gv = _train_reference(vsa, T, dh, family, p)

    def forward(q, k, v, m):
        n = q.shape[0]
        out = torch.full((n, T, d), float("nan"), device=_dev())
        lse = torch.full((n, H, T), float("nan"), device=_dev())
        vsa._lib.check(lib.vs_train_attention_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), m.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                                      n, H, T, dh, scale, SEED, SITE, p, _stream()))
        return out, lse

    out, lse = forward(q, k, v, m)
    dqkv = torch.full((B, T, 3 * d), float("nan"), device=_dev())
    scratch = torch.empty(B * H * T, device=_dev())
    vsa._lib.check(lib.vs_train_attention_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), m.data_ptr(), out.data_ptr(), dO.data_ptr(),
                                                   lse.data_ptr(), dqkv.data_ptr(), scratch.data_ptr(), B, H, T, dh, scale, SEED, SITE, p,
                                                   _stream()))
    torch.cuda.synchronize()
    e_lse = (lse.cpu().double() - lse2).abs().max().item()
    got = dict(out=(out, want), dq=(dqkv[:, :, :d], gq), dk=(dqkv[:, :, d:2 * d], gk), dv=(dqkv[:, :, 2 * d:], gv))
    _report("vs_train_attention p=%.1f" % p, dh, T, family, lse2=e_lse / LSE_TOL,
            **{n: _ratio(a, b, tol.TRAIN_GRAD_ATOL, tol.TRAIN_GRAD_RTOL) for n, (a, b) in got.items()})
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    for n, (a, b) in got.items():
        _close(a, b, n)
    assert e_lse < LSE_TOL, e_lse
    _assert_dead_keys_get_no_gradient(dqkv, mask, d, "exact")
    if p == 0.0:
        for b in range(B):
            o1, l1 = forward(_alone(q, b), _alone(k, b), _alone(v, b), _alone(m, b))
            assert torch.equal(o1[0], out[b]) and torch.equal(l1[0], lse[b]), ("alone", b, lm.first_live(T)[b])
        if family == "lead":
            b, rows = _one_hot_rows(vh, T)
            assert torch.equal(out[b].cpu(), rows), (out[b].cpu() - rows).abs().max().item()


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "fp16"])
@both_families
@pytest.mark.parametrize("dh,T", _grid((32, 64, 128), (65, 200)))
def test_train_attention_16bit(vsa, dh, T, family, f16, p):
    """attn_fwd_train_bf16 and its two backward kernels in both 16-bit types and both storage forms (in16 = 0 / 1 with bf16,
    64 / 65 with fp16), at the bounds of test_attention_forward_and_backward_kernels_bf16.  Within a type the stored form gives
    the bits of the fp32-stored one, and a second run gives the same bits.  Nothing exact is asked of the one-hot video here:
    the row constant of these kernels sits on a grid."""
    lib = vsa._lib.load()
    (q, k, v, m, dO), (_, _, _, mask, scale, _) = _device_case(T, dh, family)
    B, d = q.shape[0], H * dh
    want, lse2, _, gq, gk, gv = _train_reference(vsa, T, dh, family, p)
    dbits = None
    if p > 0:
        dbits = torch.empty(lib.vs_train_attention_dropout_bits_bytes(B, H, T), dtype=torch.uint8, device=_dev())
        vsa._lib.check(lib.vs_train_attention_dropout_bits(dbits.data_ptr(), B, H, T, SEED, SITE, p, _stream()))
    t16 = torch.float16 if f16 else torch.bfloat16
    stored = ((q * (scale * LOG2E)).to(t16).contiguous(), k.to(t16).contiguous(), v.to(t16).contiguous())
    scratch = torch.empty(B * H * T, device=_dev())

    def run(ops, in16):
        out = torch.full((B, T, d), float("nan"), device=_dev())
        lse = torch.full((B, H, T), float("nan"), device=_dev())
        dqkv = torch.full((B, T, 3 * d), float("nan"), device=_dev())
        a, b, c = (t.data_ptr() for t in ops)
        vsa._lib.check(lib.vs_train_attention_forward_bf16(a, b, c, m.data_ptr(), out.data_ptr(), lse.data_ptr(), B, H, T, dh, scale, p,
                                                           _ptr(dbits), in16, _stream()))
        vsa._lib.check(lib.vs_train_attention_backward_bf16(a, b, c, m.data_ptr(), out.data_ptr(), dO.data_ptr(), lse.data_ptr(),
                                                            dqkv.data_ptr(), scratch.data_ptr(), B, H, T, dh, scale, p, _ptr(dbits), in16,
                                                            _stream()))
        torch.cuda.synchronize()
        return out, lse, dqkv

    bit = 64 if f16 else 0
    first, again, planes = run((q, k, v), bit), run((q, k, v), bit), run(stored, bit | 1)
    out, lse, dqkv = first
    e_lse = (lse.cpu().double() - lse2).abs().max().item()
    got = dict(out=(out, want, LP_OUT), dq=(dqkv[:, :, :d], gq, LP_GRAD), dk=(dqkv[:, :, d:2 * d], gk, LP_GRAD),
               dv=(dqkv[:, :, 2 * d:], gv, LP_GRAD))
    _report("vs_train_attention_%s p=%.1f" % ("fp16" if f16 else "bf16", p), dh, T, family, lse2=e_lse / LP_LSE,
            **{n: _ratio(a, b, None, r) for n, (a, b, r) in got.items()})
    assert all(torch.isfinite(t).all() for t in first + planes)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs differ"
    assert all(torch.equal(a, b) for a, b in zip(first, planes)), "the 16-bit stored form differs from the fp32-stored one"
    for n, (a, b, r) in got.items():
        _close(a, b, n + " (16-bit)", atol=None, rtol=r)
    assert e_lse < LP_LSE, e_lse
    _assert_dead_keys_get_no_gradient(dqkv, mask, d, "16-bit")


# ---- whole model: scoring ---------------------------------------------------------------------------------------------------
MODEL = dict(d=256, L=2, B=4, T=200, wseed=51, xseed=52)
MODEL_FIRST_LIVE = (1, 64, 129, 199)      # 129: waves 0 - 3 of the split-key kernel see only dead tiles


def _model_case(vsa, heads):
    c = MODEL
    sd = vsa.synth.make_state_dict(c["d"], c["L"], c["wseed"])
    x = vsa.synth.make_features(c["B"], c["T"], c["xseed"], "randn")
    mask = torch.zeros(c["B"], c["T"], dtype=torch.bool)
    for b, f in enumerate(MODEL_FIRST_LIVE):
        mask[b, :f] = True
    m = vsa.SimNet(num_heads=heads, d_model=c["d"], num_layers=c["L"], sparsity=0.0, dropout=0.3)
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        rl, rh = oracle_forward(sd, x, mask, heads)
    return m.to(_dev()).eval(), x.to(_dev()), mask.to(_dev()), ~mask, rl, rh


def _exact_errors(m, x, md, valid, rl, rh):
    with torch.no_grad():
        logits, hidden = m(x, md)
    torch.cuda.synchronize()
    assert torch.isfinite(logits.cpu()[valid]).all() and torch.isfinite(hidden.cpu()[valid]).all()
    return (logits.cpu() - rl)[valid].abs().max().item(), (hidden.cpu() - rh)[valid].abs().max().item(), logits


@pytest.mark.parametrize("heads", [4, 2], ids=["head_dim_64", "head_dim_128"])
def test_model_scores_videos_with_masked_leading_frames(vsa, heads):
    """H 4 / H 2, d_model 256, two layers, four 200-frame videos whose first valid frame is 1, 64, 129, 199, against
    oracle_forward on the valid frames: the default kernels, and at head dim 64 the tiled and fused layer kernels
    (VS_SKINNY_ROWS = 0), the split-key latency kernel and the fp16x3 emulation, each at FP32_TOL; then every product on the bf16
    pipe (VS_LP_MIN_ROWS = 0) against the exact path at BF16_LOGIT_TOL / BF16_SCORE_TOL."""
    m, x, md, valid, rl, rh = _model_case(vsa, heads)
    results = {}
    try:
        results["default"] = _exact_errors(m, x, md, valid, rl, rh)
        exact = results["default"][2]
        if heads == 4:
            vsa._lib.set_option("VS_SKINNY_ROWS", 0)
            results["tiled"] = _exact_errors(m, x, md, valid, rl, rh)
            vsa._lib.set_option("VS_SKINNY_ROWS", -1)
            m.set_latency_mode(True)
            results["latency"] = _exact_errors(m, x, md, valid, rl, rh)
            m.set_latency_mode(False)
            m.set_compute_dtype("fp16x3")
            results["fp16x3"] = _exact_errors(m, x, md, valid, rl, rh)
            m.set_compute_dtype("fp32")
        vsa._lib.set_option("VS_LP_MIN_ROWS", 0)
        m.set_compute_dtype("bf16")
        with torch.no_grad():
            l16, _ = m(x, md)
            s16 = m.score(x, md)
        m.set_compute_dtype("fp32")
        with torch.no_grad():
            s32 = m.score(x, md)
        torch.cuda.synchronize()
    finally:
        vsa._lib.set_option("VS_SKINNY_ROWS", -1)
        vsa._lib.set_option("VS_LP_MIN_ROWS", -1)
        m.set_latency_mode(False)
        m.set_compute_dtype("fp32")
    e_logit = (l16 - exact).cpu().squeeze(-1)[valid].abs().max().item()
    e_score = (s16 - s32).cpu()[valid].abs().max().item()
    for name, (el, eh, _) in results.items():
        print("lead-mask model H %d %-8s logits %.2e hidden %.2e  (err/bound %.3f)" % (heads, name, el, eh, max(el, eh) / tol.FP32_TOL))
    print("lead-mask model H %d bf16     logits %.2e scores %.2e of the exact path  (err/bound %.3f)"
          % (heads, e_logit, e_score, max(e_logit / tol.BF16_LOGIT_TOL, e_score / tol.BF16_SCORE_TOL)))
    for name, (el, eh, _) in results.items():
        assert el < tol.FP32_TOL and eh < tol.FP32_TOL, (name, el, eh)
    assert math.isfinite(e_logit) and math.isfinite(e_score)
    assert e_logit < tol.BF16_LOGIT_TOL and e_score < tol.BF16_SCORE_TOL, (e_logit, e_score)
    if heads == 4:
        assert not torch.equal(results["latency"][2], exact), "the latency mode did not run"
