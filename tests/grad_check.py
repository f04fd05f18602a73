"""Test infrastructure (not product code): the per-tensor rules that hold one HIP training step's gradients against the
float64 explicit-mask model (tests/torch_ref.py).  Shared by the training soak (tools/fuzz_train.py) and the large-batch
tests (tests/test_hip_train_at_scale.py), so both apply the same bounds of tests/tolerances.py.

    exact fp32   per tensor, max |g - g64| <= TRAIN_GRAD_ATOL * max(1, max |g64|) and
                 <= TRAIN_GRAD_RTOL * max |g64| + 1e-6 * max(1, head_dim / 64) * (the step's largest gradient entry)
                 (the second term is the floor for analytically-zero sums - k.bias: sum_k dS = 0 per query - whose residue
                 is the rounding of head-dim dot products; measured 1.5e-8 / 6.6e-8 / 1.2e-7 / 2.3e-7 of the case's largest
                 gradient at head dim 32 / 64 / 128 / 256 over 12 cases each, 1.07e-6 once in a 200 s soak at head dim 256)
    bf16 / fp16  per tensor, relative L2 error ||g - g64|| / max(||g64||, 1e-3 * (largest entry) * sqrt(numel)) <=
                 TRAIN_LP_GRAD_L2 (bf16) / TRAIN_FP16_GRAD_L2 (fp16); the bf16 q / k projections are measured against the
                 larger of their own norm and the same layer's v projection gradient's (scaled to their size) and held to
                 TRAIN_LP_QK_L2: dS = P (dP - delta) is a DIFFERENCE, the bf16 rounding of dO and V enters at the scale of dP,
                 whatever is left after the subtraction (diffuse attention: little)."""
import tolerances as tol


def check_gradients(pairs, head_dim, lp=False):
    """pairs: [(name, got, want)] with `got` the implementation's gradient (already divided by any loss scale) and `want`
    the float64 one; lp: False (exact fp32), "bf16" or "fp16".
    Returns one (name, metric, bound, ok) per tensor: exact fp32 - metric = max |g - g64| / max |g64| and bound = the
    largest value the rule admits on that scale (a tensor whose largest entry lies under the analytically-zero floor is
    measured against the scale at which the floor equals TRAIN_GRAD_RTOL instead); low precision - metric = the relative
    L2 error and bound its limit."""
    wants = dict((k, w) for k, _g, w in pairs)
    gscale = max(w.abs().max().item() for w in wants.values())
    out = []
    for k, got, want in pairs:
        diff = got.detach().double().to(want.device) - want
        if lp:
            ref_norm = want.norm().item()
            qk = ".sa.q." in k or ".sa.k." in k
            if qk:
                wv = wants[k.split(".sa.")[0] + ".sa.v.weight"]
                ref_norm = max(ref_norm, wv.norm().item() * (want.numel() / wv.numel()) ** 0.5)
            l2 = diff.norm().item() / max(ref_norm, 1e-3 * gscale * want.numel() ** 0.5, 1e-30)
            bound = tol.TRAIN_LP_QK_L2 if (qk and lp != "fp16") else (tol.TRAIN_FP16_GRAD_L2 if lp == "fp16" else tol.TRAIN_LP_GRAD_L2)
            out.append((k, l2, bound, l2 <= bound))
            continue
        err = diff.abs().max().item()
        scale = want.abs().max().item()
        floor = 1e-6 * max(1.0, head_dim / 64.0) * gscale
        bound = min(tol.TRAIN_GRAD_ATOL * max(1.0, scale), tol.TRAIN_GRAD_RTOL * scale + floor)
        # an analytically-zero tensor (the key bias) is pure rounding: its error is stated relative to the floor's scale
        ref = scale if scale * tol.TRAIN_GRAD_RTOL >= floor else floor / tol.TRAIN_GRAD_RTOL
        out.append((k, err / max(ref, 1e-30), bound / max(ref, 1e-30), err <= bound))
    return out


def report(tag, rows):
    """One line per tensor: its worst relative error and the bound it was held to (see check_gradients)."""
    print("\n".join([tag] + ["   %-52s %.3e  (bound %.3e)%s" % (k, m, b, "" if ok else "  FAIL") for k, m, b, ok in rows]), flush=True)
