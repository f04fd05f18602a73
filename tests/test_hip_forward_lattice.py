"""GPU: the scoring forward on EVERY native shape (tests/forward_lattice_cases.py: 44 (heads, d_model) pairs) in every compute
mode, with the row thresholds pinned to 0 and at their defaults, as a padded + masked batch and as a packed ragged batch, against
the CPU oracle - and the latency mode across embedding widths.  The planner (csrc/vs_forward_plan.h) picks kernels from d_model,
head dim, mode and row count; this walks that space instead of sampling it, so a plan that names a kernel no launcher has
(packed bf16 at head dim 128 with d_model <= 256; latency mode at in_features 3072) fails here as a shape id.

Bars are those of tests/tolerances.py: FP32_TOL for fp32 and fp16x3, BF16_LOGIT_TOL / BF16_SCORE_TOL for bf16.  Every cell prints
one `forward_lattice_parity ...` line (profiles/forward_lattice_parity.txt is a run's collection of them)."""
import re

import pytest
import torch

import forward_lattice_cases as cases
import tolerances as tol
from oracle.simnet_oracle import oracle_forward

pytestmark = pytest.mark.gpu

LOGIT_TOL = {"fp32": tol.FP32_TOL, "fp16x3": tol.FP32_TOL, "bf16": tol.BF16_LOGIT_TOL}
SCORE_TOL = {"fp32": tol.FP32_TOL, "fp16x3": tol.FP32_TOL, "bf16": tol.BF16_SCORE_TOL}
BF16_NOT_EXACT = 1e-5       # a bf16 cell whose Linears are pinned to the bf16 kernels is further than this from the oracle


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture
def options(vsa):
    """set(name, value) for the library's switches; every one touched is back at its default afterwards"""
    touched = set()

    def set_option(name, value):
        touched.add(name)
        vsa._lib.set_option(name, value)

    try:
        yield set_option
    finally:
        for name in touched | set(cases.PIN_OPTIONS):
            vsa._lib.set_option(name, -1)


def _model(vsa, shape, sd, in_features=cases.IN_FEATURES):
    H, d = shape
    m = vsa.SimNet(num_heads=H, d_model=d, num_layers=cases.NUM_LAYERS, sparsity=0.0, dropout=0.3, in_features=in_features)
    m.load_state_dict(sd, strict=True)
    return m.to(_dev()).eval()


def _errors(logits, hidden, rl, rh, valid):
    """max |logit - oracle|, max |hidden - oracle| over the valid frames; everything there finite"""
    l, h = logits.cpu(), hidden.cpu()
    assert torch.isfinite(l[valid]).all() and torch.isfinite(h[valid]).all()
    return (l - rl).abs().squeeze(-1)[valid].max().item(), (h - rh).abs()[valid].max().item()


@pytest.mark.parametrize("shape", cases.NATIVE, ids=cases.shape_id)
def test_native_shape_in_every_mode_and_call_form(vsa, options, shape):
    H, d = shape
    dh = d // H
    synth = vsa.synth
    lengths = list(cases.LENGTHS)
    wseed, xseed = cases.seeds(shape)
    sd = synth.make_state_dict(d, cases.NUM_LAYERS, wseed, trained_like=True)
    x = synth.make_features(len(lengths), max(lengths), xseed, "pool5", lengths=lengths)
    mask = synth.padding_mask(x)
    assert tuple(x.shape) == (4, 257, cases.IN_FEATURES) and (~mask).sum(1).tolist() == lengths
    valid = ~mask
    with torch.no_grad():
        rl, rh = oracle_forward(sd, x, mask, H)                  # once per shape; read only below
    rs = torch.sigmoid(rl).squeeze(-1)
    # the packed form's reference: the valid rows, video after video
    rlp, rhp, rsp = rl[valid], rh[valid], rs[valid]
    all_rows = torch.ones(cases.ROWS, dtype=torch.bool)
    m = _model(vsa, shape, sd)
    dx, dm = x.to(_dev()), mask.to(_dev())
    xp = torch.cat([x[b, :t] for b, t in enumerate(lengths)], dim=0).to(_dev())
    assert xp.size(0) == cases.ROWS

    def line(mode, pin, form, text):
        print("forward_lattice_parity H=%d d=%d mode=%s pin=%d form=%s %s" % (H, d, mode, pin, form, text))

    for mode in cases.MODES:
        m.set_compute_dtype(mode)
        if dh == 256:
            assert m.attention_dtype == "fp32"                   # head dim 256 has the exact attention only, in every mode
        elif mode == "bf16":
            assert m.attention_dtype == "bf16"
        for pin in cases.PINS:
            for name in cases.PIN_OPTIONS:
                options(name, pin)
            bf16_pinned = mode == "bf16" and pin == 0            # the plan runs bf16 Linears at these row counts
            with torch.no_grad():
                logits, hidden = m(dx, dm)
                score = m.score(dx, dm)
            el, eh = _errors(logits, hidden, rl, rh, valid)
            sc = score.cpu()
            assert torch.isfinite(sc[valid]).all()
            es = (sc - rs).abs()[valid].max().item()
            line(mode, pin, "padded", "err=%.3e hidden=%.3e score=%.3e" % (el, eh, es))
            assert max(el, eh) < LOGIT_TOL[mode] and es < SCORE_TOL[mode], (mode, pin, "padded", el, eh, es)
            if bf16_pinned:
                assert el > BF16_NOT_EXACT, (mode, pin, "padded", el)

            if dh not in cases.PACKED_HEAD_DIMS:
                with pytest.raises(RuntimeError, match=re.escape(cases.PACKED_REFUSAL)):
                    m.forward_packed(xp, lengths)
                with pytest.raises(RuntimeError, match=re.escape(cases.PACKED_REFUSAL)):
                    m.score_packed(xp, lengths)
                line(mode, pin, "packed", "err=refused")
                continue
            with torch.no_grad():
                lp, hp = m.forward_packed(xp, lengths)
                sp = m.score_packed(xp, lengths)
            assert tuple(lp.shape) == (cases.ROWS, 1) and tuple(hp.shape) == (cases.ROWS, d) and tuple(sp.shape) == (cases.ROWS,)
            pl, ph = _errors(lp, hp, rlp, rhp, all_rows)
            spc = sp.cpu()
            assert torch.isfinite(spc).all()
            ps = (spc - rsp).abs().max().item()
            line(mode, pin, "packed", "err=%.3e hidden=%.3e score=%.3e" % (pl, ph, ps))
            assert max(pl, ph) < LOGIT_TOL[mode] and ps < SCORE_TOL[mode], (mode, pin, "packed", pl, ph, ps)
            if bf16_pinned:
                assert pl > BF16_NOT_EXACT, (mode, pin, "packed", pl)
            if mode == "bf16":
                continue
            # fp32 and fp16x3: a video's bits do not depend on the batch or the call form it is scored in
            row = 0
            for b, t in enumerate(lengths):
                with torch.no_grad():
                    l1, h1 = m(dx[b:b + 1, :t].contiguous())
                assert torch.equal(lp[row:row + t], logits[b, :t]) and torch.equal(hp[row:row + t], hidden[b, :t]), (mode, pin, "packed != padded", b)
                assert torch.equal(lp[row:row + t], l1[0]) and torch.equal(hp[row:row + t], h1[0]), (mode, pin, "packed != alone", b)
                row += t


@pytest.mark.parametrize("in_features", cases.LATENCY_IN_FEATURES)
@pytest.mark.parametrize("shape", cases.LATENCY_MODELS, ids=cases.shape_id)
def test_latency_mode_across_embedding_widths(vsa, options, shape, in_features):
    """set_latency_mode(True) on one 65-frame video: the oracle at FP32_TOL and the same bits twice, whether the embedding's K
    splits eight ways (in_features 1024, 2048) or keeps its default kernel (3072: a 384-wide slice is none the split-K kernel takes)."""
    H, d = shape
    synth = vsa.synth
    T = cases.LATENCY_FRAMES
    wseed, xseed = cases.latency_seeds(shape, in_features)
    sd = synth.make_state_dict(d, cases.NUM_LAYERS, wseed, in_features=in_features, trained_like=True)
    x = synth.make_features(1, T, xseed, "pool5", in_features=in_features)
    with torch.no_grad():
        rl, rh = oracle_forward(sd, x, None, H)
    valid = torch.ones(1, T, dtype=torch.bool)
    m = _model(vsa, shape, sd, in_features=in_features).set_latency_mode(True)
    dx = x.to(_dev())
    for mode in cases.LATENCY_MODES:
        m.set_compute_dtype(mode)
        with torch.no_grad():
            l1, h1 = m(dx)
            l2, h2 = m(dx)
        el, eh = _errors(l1, h1, rl, rh, valid)
        print("forward_lattice_parity H=%d d=%d mode=%s pin=-1 form=latency_in%d err=%.3e hidden=%.3e" % (H, d, mode, in_features, el, eh))
        assert max(el, eh) < tol.FP32_TOL, (mode, in_features, el, eh)
        assert torch.equal(l1, l2) and torch.equal(h1, h2), (mode, in_features, "not deterministic")
