#!/usr/bin/env python3
"""Randomised soak of the HIP TRAINING path against the float64 explicit-mask torch model (tests/torch_ref.py): random
architecture (head dim 32 / 64 / 128, d_model 128 ... 512, 1-3 layers), batch, length (1 ... 700, ragged), mask kind
(none / suffix padding / arbitrary), dropout (0 or 0.1 ... 0.5, embedding dropout sometimes), both outputs carrying
gradient.  Every case compares logits, the loss and EVERY gradient (input and parameters).

    python tools/fuzz_train.py [seconds] [seed] [bf16 | fp16]

`bf16`: the same soak under set_train_dtype("bf16") (Linear / dgrad / wgrad GEMMs and, for head dim 32 / 64, the attention
forward and backward on bf16 operands; pinned on from the first row).  The checker still shares the implementation's gates,
so what is left is smooth bf16 rounding: per tensor the relative L2 error is held to tests/tolerances.py TRAIN_LP_GRAD_L2.
The per-tensor rules live in tests/grad_check.py.  Half of the cases pin the LDS-tiled GEMMs (VS_SKINNY_ROWS = 0), so both
GEMM families run the training epilogues; the option is restored when the soak ends, also when a case fails."""
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("video-summarization_amd")
import tolerances as tol          # noqa: E402
import torch_ref                  # noqa: E402
import grad_check                 # noqa: E402  (the per-tensor gradient rules, shared with tests/test_hip_train_at_scale.py)
import test_hip_train as tht      # noqa: E402  (_library_masks)

ARCH = [(4, 256), (8, 256), (4, 128), (2, 128), (4, 512), (8, 512), (2, 64), (6, 192), (5, 320),
        # round 4: shapes embedded in the next supported one (head dim 16, 40, 36, three heads of 32, 200 -> 256) and head dim 256
        (8, 128), (5, 200), (2, 72), (3, 96), (1, 200), (1, 256)]
LENGTHS = [1, 2, 5, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 150, 200, 255, 256, 257, 320, 400, 511, 513, 700]
ATOL, RTOL = tht.ATOL, tht.RTOL          # tests/tolerances.py: TRAIN_GRAD_ATOL / TRAIN_GRAD_RTOL
# The float64 checker differentiates the SAME piecewise-linear function as the implementation: it takes the ReLU-and-
# dropout gate of every layer from the HIP forward's own activation record (a ReLU input within fp32 rounding of zero
# may fall on the other side in float64, and with millions of activations per case some do).


def run(budget, seed, progress=True, lp=False):
    """lp: False (exact fp32), True / "bf16", or "fp16" (under tests/tolerances.py's loss scale, like the reference's GradScaler)"""
    lp_name = "fp16" if lp == "fp16" else "bf16"
    S = tol.TRAIN_FP16_LOSS_SCALE if lp == "fp16" else 1.0
    dev = torch.device("cuda:0")
    if lp:
        pkg._lib.set_option("VS_TRAIN_LP_MIN_ROWS", 0)
    rng = np.random.Generator(np.random.PCG64(seed))
    torch.set_num_threads(16)
    t_end, n, worst, t_print, nrisky = time.time() + budget, 0, 0.0, time.time() + 30, 0
    try:
        while time.time() < t_end:
            case_worst, risky = _case(rng, dev, lp, lp_name, S)
            n, worst, nrisky = n + 1, max(worst, case_worst), nrisky + risky
            if progress and time.time() > t_print:
                print("  ... %d cases (%d with a ReLU input inside fp32 rounding of 0), worst relative gradient error %.2e" % (n, nrisky, worst), flush=True)
                t_print = time.time() + 30
    finally:
        pkg._lib.set_option("VS_SKINNY_ROWS", -1)
        if lp:
            pkg._lib.set_option("VS_LP_MLP_UNFUSED", -1)
            pkg._lib.set_option("VS_TRAIN_LP_MIN_ROWS", -1)
    return n, worst, nrisky


def _case(rng, dev, lp, lp_name, S):
    """One random case; raises on a violation.  Returns (its worst gradient metric, 1 if it has a ReLU input within 5e-6 of 0)."""
    H, d = ARCH[rng.integers(len(ARCH))]
    L = int(rng.integers(1, 4))
    B = int(rng.integers(1, 5))
    T = int(rng.choice(LENGTHS))
    kind = rng.choice(["none", "suffix", "random"])
    p = float(rng.choice([0.0, 0.0, 0.1, 0.3, 0.5]))
    p_embed = float(rng.choice([0.0, 0.0, 0.0, 0.25])) if p > 0 else 0.0
    hidden_w = float(rng.choice([0.0, 1e-3]))
    sd = pkg.synth.make_state_dict(d, L, int(rng.integers(1 << 30)), trained_like=bool(rng.integers(2)))
    lengths = None
    if kind == "suffix" and T > 1:
        lengths = [int(rng.integers(1, T + 1)) for _ in range(B)]
        lengths[int(rng.integers(B))] = T
    x = pkg.synth.make_features(B, T, int(rng.integers(1 << 30)), "pool5" if rng.integers(2) else "randn", lengths=lengths)
    mask = pkg.synth.padding_mask(x) if lengths is not None else (pkg.synth.random_mask(B, T, int(rng.integers(1 << 30))) if kind == "random" else None)
    target = torch.from_numpy(rng.random((B, T)).astype(np.float32))
    R = torch.from_numpy(rng.standard_normal((B, T, d)).astype(np.float32))
    # half of the cases pin the LDS-tiled GEMMs (VS_SKINNY_ROWS = 0), the other half take the latency kernels these row counts get by default
    pin = int(rng.integers(2))
    pkg._lib.set_option("VS_SKINNY_ROWS", 0 if pin else -1)
    m = pkg.SimNet(num_heads=H, d_model=d, num_layers=L, sparsity=p_embed, dropout=p)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    if lp:
        m.set_train_dtype(lp_name)
        # half of the cases pin the A-stationary GEMM (d_model 256 only; by itself it engages from 49 152 rows up)
        pkg._lib.set_option("VS_LP_MLP_UNFUSED", 2 if rng.integers(2) else -1)
    tseed = int(rng.integers(1 << 30))
    torch.manual_seed(tseed)
    seed64 = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if (p > 0 or p_embed > 0) else 0
    torch.manual_seed(tseed)
    xd = x.to(dev).requires_grad_(True)
    md = None if mask is None else mask.to(dev)
    pred, hidden = m(xd, md)
    mk = md if md is not None else torch.zeros(B, T, dtype=torch.bool, device=dev)
    loss = pkg.mse_with_mask_loss(pred, target.to(dev), mk) + hidden_w * (hidden * R.to(dev)).sum()
    gates = tht._hip_gates(pkg, m, pred, B, T, d, L, bf16=(lp_name if lp else False))      # before backward frees the activation record
    (loss * S).backward()
    masks = tht._library_masks(pkg, B, T, d, H, L, seed64, p, p_embed) if (p > 0 or p_embed > 0) else None
    params = {k: v.double().clone().requires_grad_("pos_embedding" not in k) for k, v in sd.items()}
    x64 = x.double().clone().requires_grad_(True)
    stats = {}
    rl, rh = torch_ref.forward_with_masks(params, x64, mask, H, p, p_embed, masks, stats, gates)
    sc = torch.ones(B, T, dtype=torch.float64) if mask is None else (~mask).double()
    # bf16 soak: the float64 backward starts from the SAME loss gradient as the implementation's (the loss is evaluated at
    # the HIP logits, its derivative flows into the float64 graph): a bias gradient is 2 mean(pred - target), a sum that
    # nearly cancels, and would otherwise just measure the forward's 4e-3 logit error again (held separately below)
    rl_eff = rl + (pred.detach().cpu().double() - rl).detach() if lp else rl
    rloss = (((rl_eff.squeeze(2) - target.double()) * sc) ** 2).mean() + hidden_w * (rh * R.double()).sum()
    rloss.backward()
    tag = "H=%d d=%d L=%d B=%d T=%d mask=%s p=%.2f pe=%.2f hw=%g seed=%d pin=%d" % (
        H, d, L, B, T, kind, p, p_embed, hidden_w, tseed, pin)
    valid = torch.ones(B, T, dtype=torch.bool) if mask is None else ~mask
    e = (pred.detach().cpu().double() - rl.detach())[valid].abs().max().item()
    assert e < (tol.BF16_LOGIT_TOL if lp else ATOL), "logits %.3e: %s" % (e, tag)
    # (bf16: the hidden-state term hw * sum(hidden * R) carries the forward's rounding of ~1e5 hidden values: 5 x the loss bound)
    assert abs(loss.item() - rloss.item()) < (5 * tol.TRAIN_LP_LOSS_RTOL if lp else 2e-5) * max(1.0, abs(rloss.item())), "loss: %s" % tag
    pairs = [("x", xd.grad / S, x64.grad)] + [(k, prm.grad / S, params[k].grad) for k, prm in m.named_parameters()]
    rows = grad_check.check_gradients(pairs, d // H, lp_name if lp else False)
    bad, worst = [], 0.0
    for (k, got, want), (_k, metric, _bound, ok) in zip(pairs, rows):
        if not ok:
            bad.append("%s (%.3e)" % (k, metric) if lp else k)
        if lp or want.abs().max().item() > 1e-6:
            worst = max(worst, metric)
    if bad:
        for k, got, want in pairs:
            d_ = (got.double().cpu() - want).abs()
            print("   %-55s err %.3e  max|want| %.3e  argmax %s" % (k, d_.max().item(), want.abs().max().item(),
                                                                  tuple(int(v) for v in np.unravel_index(int(d_.argmax()), d_.shape))))
        raise AssertionError("gradients %s: %s" % (bad, tag))
    return worst, int(stats["min_abs_fc1"] < 5e-6)


def main(budget, seed, lp=False):
    """Soak for `budget` seconds from `seed`; raises on the first violation (tests/test_hip_parity.py runs a fixed-seed slice)."""
    n, worst, nrisky = run(budget, seed, lp=lp)
    if lp:
        print("fuzz_train %s: %d cases clean in %.0f s (seed %d) under set_train_dtype('%s'); worst relative L2 gradient error %.2e "
              "(bound %.1e; q / k projections in the bf16 mode %.1e)" % (lp, n, budget, seed, lp, worst,
                                                                          tol.TRAIN_FP16_GRAD_L2 if lp == "fp16" else tol.TRAIN_LP_GRAD_L2, tol.TRAIN_LP_QK_L2))
        return
    print("fuzz_train: %d cases clean in %.0f s (seed %d), %d of them with a ReLU input within 5e-6 of zero (all held to "
          "%.0e: the checker shares the implementation's gate); worst relative gradient error %.2e" % (n, budget, seed, nrisky, RTOL, worst))


if __name__ == "__main__":
    main(float(sys.argv[1]) if len(sys.argv) > 1 else 120.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1,
         sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] in ("bf16", "fp16") else False)
