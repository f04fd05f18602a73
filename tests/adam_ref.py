"""The float64 restatement of ``torch.optim.Adam`` / ``AdamW`` that the optimizer tests use as the truth
(tests/test_optim_host.py holds it against torch's own CPU Adam; tests/test_hip_optim.py measures torch's device Adam
and the HIP kernel against it).  A test helper: nothing here is product code."""
import math

import torch


def adam_ref64(p0, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, grad_scale=None,
               state=None):
    """``p0``: the fp32 start values; ``grads``: one fp32 gradient per step (as the optimizer sees it, i.e. still scaled
    when ``grad_scale`` is given); ``lr``: a float or one float per step.  ``state``: (m, v, t) to continue from.
    Everything is carried in float64 and never rounded.  Returns (p, m, v, t)."""
    b1, b2 = betas
    p = p0.detach().double().cpu().clone()
    if state is None:
        m, v, t = torch.zeros_like(p), torch.zeros_like(p), 0
    else:
        m, v, t = state[0].double().cpu().clone(), state[1].double().cpu().clone(), int(state[2])
    for i, g in enumerate(grads):
        step_lr = lr[i] if isinstance(lr, (list, tuple)) else lr
        g = g.detach().double().cpu()
        if grad_scale is not None:
            g = g / float(grad_scale)
        t += 1
        if decoupled:
            p = p * (1.0 - step_lr * weight_decay)
        elif weight_decay != 0:
            g = g + weight_decay * p
        m = m + (1.0 - b1) * (g - m)
        v = b2 * v + (1.0 - b2) * g * g
        p = p - (step_lr / (1.0 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v, t


def ulp32(x: float) -> float:
    """spacing of fp32 at |x|"""
    x = abs(float(x))
    if x == 0.0:
        return 2.0 ** -149
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


def distances(p, m, v, ref):
    """(max |p - p_ref|, max |m - m_ref| / max |m_ref|, max |v - v_ref| / max |v_ref|) of one tensor against adam_ref64's
    result; the m / v measures are relative to the tensor's largest entry (0 when that is 0 and the tensors agree)."""
    pr, mr, vr = ref[0], ref[1], ref[2]
    dp = (p.detach().double().cpu() - pr).abs().max().item()

    def rel(a, r):
        d = (a.detach().double().cpu() - r).abs().max().item()
        big = r.abs().max().item()
        return d / big if big > 0 else (0.0 if d == 0 else float("inf"))
    return dp, rel(m, mr), rel(v, vr)
