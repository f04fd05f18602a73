"""GPU tests of the HIP TRAINING step at the batch sizes real training runs, against float64.

Above VS_SKINNY_ROWS frames (16 384 by default) every training GEMM leaves the skinny latency kernels for the LDS-tiled
persistent gemm_nt_128, whose 256-row ("wide") form starts at 512 tiles: the fc1 + ReLU + dropout epilogue, the gated fc2
dgrad and the dgrads adding the residual gradient then run in code the small-batch goldens never reach.  The row kernels
(LayerNorm backward, column sums) saturate their 512-block grid above 2 048 rows and the masked-MSE loss its 256-block grid
above 65 536 elements.  Each case below runs one training step of SimNet and holds the loss, the logits, dx and every
parameter gradient to a float64 restatement of the model (tests/torch_ref.py) that takes the library's own dropout masks
and the implementation's ReLU-and-dropout gates, under the soak's per-tensor rules (tests/grad_check.py).

The float64 reference runs on the device in chunks of at most CHUNK videos: each chunk's loss is its sum of squared
errors over the FULL B * T, so the chunk gradients add up to the batch's.  Case (a) also runs it on the CPU once, which
shows the device reference is sound."""
import numpy as np
import pytest
import torch

import grad_check
import tolerances as tol
import torch_ref
from test_hip_train import _hip_gates, _library_masks

pytestmark = pytest.mark.gpu
CHUNK = 8          # videos per float64 chunk: at T = 1 024 one layer's attention probabilities are 270 MB per chunk


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _model(vsa, sd, H, d, L, p, p_embed):
    m = vsa.SimNet(num_heads=H, d_model=d, num_layers=L, sparsity=p_embed, dropout=p)
    m.load_state_dict(sd, strict=True)
    return m.to(_dev()).train()


def _hip_step(vsa, m, H, d, L, x, mask, target, R, hidden_w, lp, tseed):
    """One training step of the HIP model (gradients left in m's parameters).  Returns the logits, the loss, the
    gradients (divided by the fp16 mode's loss scale), the gates of every layer and the dropout seed the step drew."""
    dev = _dev()
    B, T = x.shape[:2]
    S = tol.TRAIN_FP16_LOSS_SCALE if lp == "fp16" else 1.0
    torch.manual_seed(tseed)
    seed64 = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())       # what the training forward draws
    torch.manual_seed(tseed)
    m.zero_grad(set_to_none=True)
    xd = x.to(dev).requires_grad_(True)
    md = mask.to(dev)
    pred, hidden = m(xd, md)
    assert m.last_train_dtype == (lp or "fp32")
    loss = vsa.mse_with_mask_loss(pred, target.to(dev), md)
    if hidden_w:
        loss = loss + hidden_w * (hidden * R.to(dev)).sum()
    gates = _hip_gates(vsa, m, pred, B, T, d, L, bf16=lp or False)        # before backward frees the activation record
    (loss * S).backward()
    torch.cuda.synchronize()
    grads = [("x", xd.grad / S)] + [(k, prm.grad / S) for k, prm in m.named_parameters()]
    return pred.detach(), loss.item(), grads, gates, seed64


def _reference(sd, H, x, mask, target, R, p, p_embed, hidden_w, masks, gates, dev, pred=None, chunk=CHUNK):
    """float64 loss, logits and gradients {name: grad} of the step, on `dev`, `chunk` videos at a time.  pred (the
    low-precision modes): the backward starts from the loss gradient at the implementation's logits (the soak's rl_eff)."""
    B, T = x.shape[:2]
    params = {k: v.double().to(dev).requires_grad_("pos_embedding" not in k) for k, v in sd.items()}
    logits = torch.empty(B, T, 1, dtype=torch.float64, device=dev)
    dx, loss = [], 0.0
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        xc = x[sl].double().to(dev).requires_grad_(True)
        mc = mask[sl].to(dev)
        mk = None if masks is None else {k: v[sl].to(dev) for k, v in masks.items()}        # the hash is indexed by global video
        gt = {k: v[sl].to(dev) for k, v in gates.items()}
        rl, rh = torch_ref.forward_with_masks(params, xc, mc, H, p, p_embed, mk, None, gt)
        rl_eff = rl + (pred[sl].double().to(dev) - rl).detach() if pred is not None else rl
        closs = (((rl_eff.squeeze(2) - target[sl].double().to(dev)) * (~mc).double()) ** 2).sum() / (B * T)
        if hidden_w:
            closs = closs + hidden_w * (rh * R[sl].double().to(dev)).sum()
        closs.backward()
        loss += closs.item()
        logits[sl] = rl.detach()
        dx.append(xc.grad)
        del xc, mk, gt, rl, rh, rl_eff, closs
    grads = {"x": torch.cat(dx)}
    grads.update((k, v.grad) for k, v in params.items() if v.requires_grad)
    return loss, logits, grads


def _check_step(tag, vsa, sd, H, d, x, mask, target, R, p, p_embed, hidden_w, lp, step, masks):
    """Hold one HIP step (the output of _hip_step) to the float64 reference; prints every tensor's worst error and bound."""
    pred, loss, grads, gates, _seed = step
    dev = _dev()
    rloss, rlogits, rgrads = _reference(sd, H, x, mask, target, R, p, p_embed, hidden_w, masks, gates, dev,
                                        pred=pred if lp else None)
    valid = ~mask.to(dev)
    e_logit = (pred.double() - rlogits)[valid].abs().max().item()
    e_loss = abs(loss - rloss) / max(1.0, abs(rloss))
    logit_bound = tol.BF16_LOGIT_TOL if lp else tol.FP32_TOL
    # (low precision: the hidden-state term carries the forward's rounding of ~1e5 hidden values - the soak's 5 x the loss bound)
    loss_bound = 5 * tol.TRAIN_LP_LOSS_RTOL if lp else 2e-5
    rows = grad_check.check_gradients([(k, g, rgrads[k]) for k, g in grads], d // H, lp)
    grad_check.report("%s: logits max abs err %.3e (bound %.1e), loss rel err %.3e (bound %.1e); per tensor, %s:" % (
        tag, e_logit, logit_bound, e_loss, loss_bound,
        "relative L2 error" if lp else "max abs err / max |g64|"), rows)
    assert e_logit < logit_bound, "%s: logits %.3e" % (tag, e_logit)
    assert e_loss < loss_bound, "%s: loss %.9g vs %.9g" % (tag, loss, rloss)
    bad = [k for k, _m, _b, ok in rows if not ok]
    assert not bad, "%s: gradients %s" % (tag, bad)
    return rgrads, rlogits, rloss


def _inputs(vsa, B, T, d, seed, lengths=None, randmask=False):
    x = vsa.synth.make_features(B, T, seed, "pool5", lengths)
    if lengths is not None:
        mask = vsa.synth.padding_mask(x)
    elif randmask:
        mask = vsa.synth.random_mask(B, T, seed + 1)
    else:
        mask = torch.zeros(B, T, dtype=torch.bool)
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    target = torch.from_numpy(rng.random((B, T)).astype(np.float32))
    R = torch.from_numpy(rng.standard_normal((B, T, d)).astype(np.float32))
    return x, mask, target, R


def _ragged(B, T, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = [int(v) for v in rng.integers(T // 4, T + 1, size=B)]
    lengths[int(rng.integers(B))] = T
    return lengths


# case: H, d, L, B, T, lengths / mask, dropout, embedding dropout, hidden-state weight, modes
CASES = {
    # skinny GEMMs; 2 800 rows: the LayerNorm-backward / column-sum row kernels past 2 048 rows (grid saturated)
    "a_B4xT700_suffix": dict(H=4, d=256, L=2, B=4, T=700, lengths=[700, 650, 413, 97], p=0.3, p_embed=0.0, hidden_w=0.0,
                             modes=(False,)),
    # 17 000 rows: tiled GEMMs, wide tiles for N = 1 024 (fc1 EPI_RELU_DROP, fc2 dgrad EPI_GATE, dx)
    "b_B17xT1000_ragged": dict(H=4, d=256, L=2, B=17, T=1000, lengths=_ragged(17, 1000, 5), p=0.3, p_embed=0.25, hidden_w=1e-3,
                               modes=(False,)),
    # the bench batch (65 536 rows, L = 2 instead of 4: every layer runs the same kernels): wide tiles for every N, persistent
    # tile loops, the MSE loss past 65 536 elements; bf16 here also runs the A-stationary MLP GEMM (from 49 152 rows)
    "c_B64xT1024_bench": dict(H=4, d=256, L=2, B=64, T=1024, lengths=None, p=0.3, p_embed=0.0, hidden_w=0.0,
                              modes=(False, "bf16", "fp16")),
    # the reference's default width (head dim 128): tiled N = 2 048 / K = 512 shapes and the kw64 bf16 form
    "d_d512_B18xT1000_randmask": dict(H=4, d=512, L=1, B=18, T=1000, lengths=None, randmask=True, p=0.3, p_embed=0.0,
                                      hidden_w=0.0, modes=(False, "bf16")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_training_step_at_scale_matches_float64(vsa, name):
    c = CASES[name]
    H, d, L, B, T, p, p_embed, hidden_w = (c[k] for k in ("H", "d", "L", "B", "T", "p", "p_embed", "hidden_w"))
    sd = vsa.synth.make_state_dict(d, L, 31)
    x, mask, target, R = _inputs(vsa, B, T, d, 32, c["lengths"], c.get("randmask", False))
    if name.startswith("c_"):
        mask[5, 900:] = True
    masks = None
    for lp in c["modes"]:
        m = _model(vsa, sd, H, d, L, p, p_embed)
        if lp:
            m.set_train_dtype(lp)
        step = _hip_step(vsa, m, H, d, L, x, mask, target, R, hidden_w, lp, tseed=33)
        del m
        if masks is None:          # one seed for every mode: the same masks
            masks = _library_masks(vsa, B, T, d, H, L, step[4], p, p_embed)
        rgrads, rlogits, rloss = _check_step("%s [%s]" % (name, lp or "fp32"), vsa, sd, H, d, x, mask, target, R, p, p_embed,
                                             hidden_w, lp, step, masks)
        if name.startswith("a_"):
            # the device float64 reference against the same reference on the CPU (one chunk)
            closs, clogits, cgrads = _reference(sd, H, x, mask, target, R, p, p_embed, hidden_w, masks, step[3],
                                                torch.device("cpu"), chunk=B)
            gscale = max(g.abs().max().item() for g in cgrads.values())
            assert abs(rloss - closs) <= 1e-10 * abs(closs)
            assert (rlogits.cpu() - clogits).abs().max().item() <= 1e-10 * clogits.abs().max().item()
            worst = 0.0
            for k, want in cgrads.items():
                # relative to the tensor's largest entry; the analytically-zero key bias (pure float64 rounding) against
                # 1e-3 of the step's largest gradient, the floor grad_check's relative L2 rule uses
                scale = max(want.abs().max().item(), 1e-3 * gscale)
                err = (rgrads[k].cpu() - want).abs().max().item()
                assert err <= 1e-10 * scale, "device vs CPU float64 reference, %s: %.3e of %.3e" % (k, err, scale)
                worst = max(worst, err / scale)
            print("%s: device float64 reference vs CPU: worst gradient error %.2e relative (bound 1e-10)" % (name, worst))
        del step, rgrads, rlogits
        torch.cuda.empty_cache()


def test_batches_crossing_the_skinny_threshold_between_adam_steps(vsa):
    """One module, four Adam steps alternating 320 and 17 000 frames, so the GEMM family changes every step while the
    parameters change between steps: the weight-layout copies each family reads (the transposed and fragment-major
    copies, re-packed by version stamp) must follow.  Every step's gradients against float64 at the current parameters."""
    H, d, L, p = 4, 256, 2, 0.3
    m = _model(vsa, vsa.synth.make_state_dict(d, L, 41), H, d, L, p, 0.0)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    for i, (B, T) in enumerate([(1, 320), (17, 1000), (1, 320), (17, 1000)]):
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        x, mask, target, R = _inputs(vsa, B, T, d, 50 + 3 * i, _ragged(B, T, 60 + i) if B > 1 else None)
        step = _hip_step(vsa, m, H, d, L, x, mask, target, R, 0.0, False, tseed=70 + i)
        masks = _library_masks(vsa, B, T, d, H, L, step[4], p, 0.0)
        _check_step("Adam step %d, %d frames" % (i, B * T), vsa, sd, H, d, x, mask, target, R, p, 0.0, 0.0, False, step, masks)
        opt.step()
        del step, masks
    torch.cuda.empty_cache()
