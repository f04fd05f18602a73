"""GPU: gradient-norm clipping (include/vs_optim.h: vs_grad_norm*, vs_grad_scale_tensors; optim.py: Adam(max_grad_norm=...),
clip_grad_norm_, grad_norm).

Bounds, from the formats:
* the norm: every square is exact in double, the double sum of n terms is off by about n 2^-53 relative, the square root and
  the division by the scale by 2^-53 each, and ONE rounding to fp32 follows: one fp32 spacing (``ulp32``) of the float64
  restatement.  The max norm is a selection and one exact division by a power of two: exact.
* ``clip_grad_norm_``: the coefficient is the float64 one to about 1e-10 before its rounding to fp32 (2^-24), the product
  rounds once more (2^-24): 2^-22 relative with room, plus 2^-149 where the product is subnormal.
* the fused step: the bar of tests/test_hip_optim.py (``_assert_bar``: at most twice torch's own distance to float64), with
  torch's own sequence - unscale_, clip_grad_norm_, torch.optim.Adam - as the yardstick."""
import copy
import math

import pytest
import torch

from adam_ref import adam_ref64, ulp32
from test_hip_optim import DEV, UpdateCounter, _assert_bar, _backward, _batch, _fresh_copy, _simnet

pytestmark = pytest.mark.gpu
INF = float("inf")
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8193]


# ---- the norm ------------------------------------------------------------------------------------------------------------
def _wide(n, gen):
    """magnitudes from 1e-12 to 1e12, both signs"""
    return torch.randn(n, generator=gen) * 10.0 ** (torch.rand(n, generator=gen) * 24 - 12)


@pytest.fixture(scope="module")
def norm_case():
    """70 tensors (two norm launches): the edge sizes, one gradient 4 bytes off a 16-byte boundary, small ones to fill up,
    plus one parameter without a gradient.  Host fp32 values, built once and left unchanged."""
    gen = torch.Generator().manual_seed(2024)
    sizes = SIZES + [4099] + [7 + 13 * i for i in range(61)]
    assert len(sizes) == 70
    vals = [_wide(n, gen) for n in sizes]
    vals[4][-1], vals[6][0] = 1e12, -1e-12                      # both ends of the range are present
    sumsq = sum(float((v.double() ** 2).sum()) for v in vals)
    return dict(sizes=sizes, vals=vals, l2=math.sqrt(sumsq), mx=max(float(v.abs().max()) for v in vals))


def _params_of(case, scale=1.0):
    params = []
    for i, v in enumerate(case["vals"]):
        p = torch.nn.Parameter(torch.zeros(v.numel(), device=DEV))
        if i == 8:
            buf = torch.zeros(v.numel() + 8, device=DEV)
            buf[1:1 + v.numel()] = v.to(DEV) * scale
            p.grad = buf[1:1 + v.numel()]                       # contiguous, misaligned
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = v.to(DEV) * scale
        params.append(p)
    params.insert(3, torch.nn.Parameter(torch.zeros(11, device=DEV)))      # no gradient: skipped
    return params


@pytest.mark.parametrize("scale", [None, 65536.0])
def test_norm_is_within_one_fp32_spacing_of_float64(vsa, norm_case, scale):
    params = _params_of(norm_case, scale or 1.0)                # a power-of-two scale: the scaled gradients are exact
    if scale is None:
        l2, mx = vsa.grad_norm(params), vsa.grad_norm(params, INF)
        again = vsa.grad_norm(params)
    else:
        # with a scale the entry is the optimizer's: measure only (max_grad_norm = inf), lr = 0 keeps the step a no-op
        gs = torch.full((), scale, device=DEV)
        outs = []
        for kind in (2.0, INF, 2.0):
            opt = vsa.Adam(params, lr=0.0, max_grad_norm=INF, grad_norm_type=kind)
            opt.grad_scale = gs
            opt.step()
            outs.append(opt.last_grad_norm.clone())
        l2, mx, again = outs
    assert l2.device == DEV and l2.dtype == torch.float32 and l2.dim() == 0
    print("L2 norm %.9e (float64 %.9e, spacing %.3e)  max norm %.9e" % (float(l2), norm_case["l2"], ulp32(norm_case["l2"]), float(mx)))
    assert abs(float(l2) - norm_case["l2"]) <= ulp32(norm_case["l2"])
    assert float(mx) == norm_case["mx"]
    assert torch.equal(l2, again)                                # bit-equal, call to call


def test_norm_does_not_depend_on_alignment_or_on_the_split_into_tensors(vsa, norm_case):
    """a chunk's partial depends on its elements alone and lands at the chunk's global index: the same data 3 floats off
    its alignment, or cut into tensors at chunk boundaries, gives the same bits"""
    lib, L = vsa._lib.load(), vsa._lib
    vals = norm_case["vals"]
    aligned = [v.to(DEV) for v in vals]
    shifted = []
    for v in vals:
        buf = torch.zeros(v.numel() + 8, device=DEV)
        buf[3:3 + v.numel()] = v.to(DEV)
        shifted.append(buf[3:3 + v.numel()])
    cut = []
    for t in aligned:                                            # 8193 -> 4096 + 4096 + 1, 4097 -> 4096 + 1, ...
        cut.extend(t.split(4096))
    assert len(cut) == len(aligned) + 4                          # 74 tensors: the launches split elsewhere, too
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def measure(tensors, kind=0):
        tab = (L.GradTensor * (2 * len(tensors)))()
        for i, t in enumerate(tensors):
            tab[2 * i].g, tab[2 * i].n = t.data_ptr(), t.numel()                # every other entry stays NULL / 0: skipped
        ws = torch.empty((lib.vs_grad_norm_workspace_bytes(tab, len(tab)),), dtype=torch.uint8, device=DEV)
        out = torch.empty((4,), device=DEV)
        L.check(lib.vs_grad_norm_tensors(tab, len(tab), kind, 1.0, None, out.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return out
    a = measure(aligned)
    assert torch.equal(a, measure(shifted)) and torch.equal(a, measure(cut))
    assert torch.equal(measure(aligned, 1), measure(shifted, 1))
    assert not torch.equal(a[0], measure(aligned[:64])[0])       # (the tensors of the second launch do count)
    norm, coef, div, zero = a.tolist()
    coef64 = 1.0 / (norm_case["l2"] + 1e-6)
    assert abs(coef - coef64) <= ulp32(coef64) and abs(div - 1.0 / coef64) <= ulp32(1.0 / coef64) and zero == 0.0


# ---- clip_grad_norm_ -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [2.0, INF])
def test_clip_grad_norm_above_and_within_the_threshold(vsa, norm_case, kind):
    truth = norm_case["l2"] if kind == 2.0 else norm_case["mx"]
    # above: max_norm = a third of the norm (a coefficient that is no power of two: every product rounds)
    params = _params_of(norm_case)
    max_norm = truth / 3.0
    ret = vsa.clip_grad_norm_(params, max_norm, norm_type=kind)
    assert abs(float(ret) - truth) <= (ulp32(truth) if kind == 2.0 else 0.0)
    coef64 = max_norm / (truth + 1e-6)
    worst = 0.0
    grads = [p.grad for p in params if p.grad is not None]
    for g, v in zip(grads, norm_case["vals"]):
        want = v.double() * coef64
        err = (g.double().cpu() - want).abs()
        bound = want.abs() * 2.0 ** -22 + 2.0 ** -149
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all())
    print("norm_type %s: worst element error %.3f of the bound" % (kind, worst))
    # within: the gradients keep their bits and the norm is still returned
    params = _params_of(norm_case)
    before = [p.grad.clone() for p in params if p.grad is not None]
    ret = vsa.clip_grad_norm_(params, 2.0 * truth, norm_type=kind)
    assert abs(float(ret) - truth) <= (ulp32(truth) if kind == 2.0 else 0.0)
    assert all(torch.equal(a, p.grad) for a, p in zip(before, [p for p in params if p.grad is not None]))


def test_free_functions_refuse_on_the_device(vsa):
    p = torch.nn.Parameter(torch.zeros(6, 4, device=DEV))
    p.grad = torch.ones(4, 6, device=DEV).t()
    assert not p.grad.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        vsa.clip_grad_norm_([p], 1.0)
    assert torch.equal(p.grad, torch.ones(6, 4, device=DEV))
    h = torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.float16))
    h.grad = torch.ones(8, device=DEV, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="fp32"):
        vsa.grad_norm([h])
    s = torch.nn.Parameter(torch.zeros(8, 2, device=DEV))
    s.grad = torch.sparse_coo_tensor(torch.tensor([[1], [1]]), torch.tensor([3.0]), (8, 2)).to(DEV)
    with pytest.raises(RuntimeError, match="sparse"):
        vsa.clip_grad_norm_([s], 1.0)
    with pytest.raises(RuntimeError, match="sparse"):
        opt = vsa.Adam([s], max_grad_norm=1.0)
        opt.step()


# ---- the fused step ----------------------------------------------------------------------------------------------------------
def _grads64(params):
    return [None if p.grad is None else p.grad.detach().double().cpu() for p in params]


def _norm64(grads, scale=1.0):
    return math.sqrt(sum(float((g * g).sum()) for g in grads if g is not None)) / scale


def _state_of(opt, params):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), opt.state[p]["step"].clone()) for p in params]


@pytest.mark.parametrize("with_scaler", [False, True])
def test_fused_step_within_the_threshold_is_bit_equal_to_no_clipping(vsa, with_scaler):
    batch = _batch(vsa, 2, 65, 5, [65, 41])
    x, mask, _ = batch
    results = []
    for clip in (False, True):
        model = _simnet(vsa, L=2)
        opt = vsa.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5).attach(model)
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0) if with_scaler else None
        for it in range(2):
            _backward(vsa, model, opt, batch, 30 + it, scaler)
            if clip:
                measured = _norm64(_grads64(model.parameters()), 1024.0 if with_scaler else 1.0)
                opt.max_grad_norm = 10.0 * measured
            if scaler is not None:
                scaler.step(opt)
                scaler.update()
            else:
                opt.step()
            if clip:
                assert abs(float(opt.last_grad_norm) - measured) <= ulp32(measured)
        model.eval()
        with torch.no_grad():
            logits = model(x, mask)[0].clone()
        results.append((_state_of(opt, list(model.parameters())), logits))
    (plain, logits0), (clipped, logits1) = results
    for a, b in zip(plain, clipped):
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert float(plain[0][3]) == 2 and torch.equal(logits0, logits1)


@pytest.mark.parametrize("stage", ["ready", "unscaled"])
def test_fused_step_above_the_threshold_against_float64_and_torch(vsa, stage):
    """three steps with max_grad_norm = a quarter of each step's measured norm; READY: the scale is still on the gradients
    when the optimizer sees them; unscaled: scaler.unscale_(optim) ran first"""
    scale = 1024.0
    model = _simnet(vsa, L=2)
    params = list(model.parameters())
    opt = vsa.Adam(params, lr=1e-3, weight_decay=1e-5, max_grad_norm=1.0).attach(model)
    scaler = torch.amp.GradScaler("cuda", init_scale=scale)
    clones = [p.detach().clone().requires_grad_() for p in params]
    theirs = torch.optim.Adam(clones, lr=1e-3, weight_decay=1e-5)
    their_scaler = torch.amp.GradScaler("cuda", init_scale=scale)
    their_scaler.scale(torch.zeros((), device=DEV))
    batch = _batch(vsa, 2, 65, 5, [65, 41])
    ref = [None] * len(params)
    for it in range(3):
        _backward(vsa, model, opt, batch, 40 + it, scaler)
        for c, p in zip(clones, params):
            c.grad = p.grad.detach().clone()                    # torch's sequence starts from the same scaled gradients
        g64 = [g / scale for g in _grads64(params)]             # the float64 truth: unscaled (exact), clipped in float64
        norm64 = _norm64(g64)
        max_norm = 0.25 * norm64
        coef64 = min(1.0, max_norm / (norm64 + 1e-6))
        for i, (p, g) in enumerate(zip(params, g64)):
            st = ref[i]
            ref[i] = adam_ref64(p.detach() if st is None else st[0], [g * coef64], 1e-3, weight_decay=1e-5, state=None if st is None else st[1:])
        # native
        opt.max_grad_norm = max_norm
        if stage == "unscaled":
            scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()
        assert abs(float(opt.last_grad_norm) - norm64) <= ulp32(norm64)
        # torch: unscale_, clip_grad_norm_, torch.optim.Adam
        their_scaler.unscale_(theirs)
        torch.nn.utils.clip_grad_norm_(clones, max_norm)
        their_scaler.step(theirs)
        their_scaler.update()
    native = [(p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in params]
    torch_ = [(c, theirs.state[c]["exp_avg"], theirs.state[c]["exp_avg_sq"]) for c in clones]
    assert all(float(opt.state[p]["step"]) == 3 == float(theirs.state[c]["step"]) for p, c in zip(params, clones))
    _assert_bar("clipped to 0.25 of the norm, %s" % stage, native, torch_, ref)
    # write-through held: the next forward is a fresh copy's
    x, mask, _ = batch
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(x, mask)[0], _fresh_copy(vsa, model).eval()(x, mask)[0])


def test_overflow_with_clipping_changes_nothing(vsa):
    model = _simnet(vsa, L=1)
    params = list(model.parameters())
    opt = vsa.Adam(params, lr=1e-3, weight_decay=1e-5, max_grad_norm=0.5).attach(model)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    batch = _batch(vsa, 2, 65, 5, [65, 41])
    _backward(vsa, model, opt, batch, 1, scaler)
    scaler.step(opt)
    scaler.update()
    assert math.isfinite(float(opt.last_grad_norm))
    before = _state_of(opt, params)
    x, mask, _ = batch
    model.eval()
    with torch.no_grad():
        before_scores = model(x, mask)[0].clone()
    _backward(vsa, model, opt, batch, 2, scaler)
    model.encoder.module_list[0].mlp.fc1.weight.grad.view(-1)[12345] = INF
    scaler.step(opt)                                             # found_inf is set by the scaler's own check
    scaler.update()
    assert scaler.get_scale() == 512.0
    assert not math.isfinite(float(opt.last_grad_norm))
    for (p0, m0, v0, s0), p in zip(before, params):
        st = opt.state[p]
        assert torch.equal(p, p0) and torch.equal(st["exp_avg"], m0) and torch.equal(st["exp_avg_sq"], v0) and torch.equal(st["step"], s0)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(x, mask)[0], before_scores)     # the packed copy too
    # the next clean step equals that of a fresh optimizer that starts from this state
    twin = _fresh_copy(vsa, model)
    twin_params = list(twin.parameters())
    fresh = vsa.Adam(twin_params, lr=1e-3, weight_decay=1e-5, max_grad_norm=0.5).attach(twin)
    fresh.load_state_dict(copy.deepcopy(opt.state_dict()))      # (a plain load aliases the live state until the first step)
    fresh.max_grad_norm = 0.5
    fresh_scaler = torch.amp.GradScaler("cuda", init_scale=512.0)
    _backward(vsa, model, opt, batch, 3, scaler)
    _backward(vsa, twin, fresh, batch, 3, fresh_scaler)
    scaler.step(opt)
    fresh_scaler.step(fresh)
    assert math.isfinite(float(opt.last_grad_norm)) and torch.equal(opt.last_grad_norm, fresh.last_grad_norm)
    for a, b in zip(_state_of(opt, params), _state_of(fresh, twin_params)):
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert float(opt.state[params[0]]["step"]) == 2


def test_clipped_scaler_step_does_not_synchronise_the_host(vsa):
    model = _simnet(vsa, L=1)
    batch = _batch(vsa, 2, 65, 5, [65, 41])
    native = vsa.Adam(model.parameters(), lr=1e-4, max_grad_norm=1.0).attach(model)
    theirs = torch.optim.Adam(model.parameters(), lr=1e-4)
    for opt in (native, theirs):                                           # warm-up: state and buffers allocated, plans built
        scaler = torch.amp.GradScaler("cuda")
        _backward(vsa, model, opt, batch, 1, scaler)
        scaler.step(opt)
        scaler.update()
    raised = {}
    for name, opt in (("torch", theirs), ("native", native)):
        scaler = torch.amp.GradScaler("cuda")
        _backward(vsa, model, opt, batch, 2, scaler)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            scaler.step(opt)
            raised[name] = False
        except RuntimeError:
            raised[name] = True
        finally:
            torch.cuda.set_sync_debug_mode("default")
    if raised["torch"]:
        assert raised["native"] is False
        return
    scaler = torch.amp.GradScaler("cuda")
    _backward(vsa, model, native, batch, 3, scaler)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        scaler.step(native)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    assert not [n for n in names if "dtoh" in n.lower().replace(" ", "") or "DeviceToHost" in n], names


# ---- groups, write-through, the generic entry, AdamW ------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Adam", "AdamW"])
def test_two_groups_share_one_global_norm_and_write_through_holds(vsa, monkeypatch, cls):
    model = _simnet(vsa)
    last = model.encoder.module_list[-1]
    loose = torch.nn.Parameter(torch.zeros(9, device=DEV))                  # in a group, never gets a gradient
    groups = [dict(params=list(model.final_layer.parameters()) + [loose], lr=1e-3), dict(params=list(last.parameters()))]
    # (no L2 decay for Adam, so that exp_avg after one step is a function of the clipped gradient alone; AdamW's is decoupled)
    opt = getattr(vsa, cls)(groups, lr=1e-4, weight_decay=1e-2 if cls == "AdamW" else 0.0, max_grad_norm=1.0).attach(model)
    batch = _batch(vsa, 2, 65, 5, [65, 41])
    counter = None
    for it in range(3):
        _backward(vsa, model, opt, batch, 10 + it)
        both = [p for g in opt.param_groups for p in g["params"]]
        norm64 = _norm64(_grads64(both))
        one = _norm64(_grads64(opt.param_groups[0]["params"]))
        opt.max_grad_norm = 0.3 * norm64
        before = [p.detach().clone() for p in both]
        g64 = _grads64(both)
        opt.step()
        if counter is None:
            counter = UpdateCounter(vsa, monkeypatch)
        assert abs(float(opt.last_grad_norm) - norm64) <= ulp32(norm64) < abs(one - norm64)      # the global norm, not a group's
        if it == 0:
            # after the first step exp_avg = (1 - beta1) * the gradient the kernel used: the globally clipped one
            for p, g in zip(both, g64):
                if g is not None:
                    coef = 0.3 * norm64 / (norm64 + 1e-6)
                    m = opt.state[p]["exp_avg"].double().cpu()
                    assert torch.allclose(m, 0.1 * g * coef, rtol=2.0 ** -20, atol=1e-30)
    assert loose not in opt.state and torch.equal(loose.detach(), torch.zeros(9, device=DEV))
    x, mask, _ = batch
    model.eval()
    with torch.no_grad():
        live = model(x, mask)
        fresh = _fresh_copy(vsa, model).eval()(x, mask)
    assert torch.equal(live[0], fresh[0]) and torch.equal(live[1], fresh[1])
    assert counter.n == 0                                                    # write-through: nothing re-packed


def test_embedded_model_clips_through_the_generic_entry(vsa):
    model = vsa.SimNet(num_heads=8, d_model=128, num_layers=2, sparsity=0.0, dropout=0.0).to(DEV)
    assert model._plan is not None
    opt = vsa.Adam(model.parameters(), lr=3e-4, max_grad_norm=1.0).attach(model)
    shadow_params = [p.detach().clone().requires_grad_() for p in model.parameters()]
    theirs = torch.optim.Adam(shadow_params, lr=3e-4)
    batch = _batch(vsa, 2, 65, 5, [65, 41])
    ref = [None] * len(shadow_params)
    params = list(model.parameters())
    for it in range(3):
        _backward(vsa, model, opt, batch, 10 + it)
        g64 = _grads64(params)
        norm64 = _norm64(g64)
        max_norm = 0.25 * norm64
        coef64 = max_norm / (norm64 + 1e-6)
        for i, (p, c, g) in enumerate(zip(params, shadow_params, g64)):
            c.grad = p.grad.detach().clone()
            st = ref[i]
            ref[i] = adam_ref64(p.detach() if st is None else st[0], [g * coef64], 3e-4, state=None if st is None else st[1:])
        opt.max_grad_norm = max_norm
        opt.step()
        torch.nn.utils.clip_grad_norm_(shadow_params, max_norm)
        theirs.step()
        assert abs(float(opt.last_grad_norm) - norm64) <= ulp32(norm64)
    _assert_bar("embedded d_model 128 / 8 heads, clipped",
                [(p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in params],
                [(c, theirs.state[c]["exp_avg"], theirs.state[c]["exp_avg_sq"]) for c in shadow_params], ref)
    x, mask, _ = batch
    model.eval()
    fresh = vsa.SimNet(num_heads=8, d_model=128, num_layers=2, sparsity=0.0, dropout=0.0).to(DEV)
    fresh.load_state_dict(model.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(model(x, mask)[0], fresh.eval()(x, mask)[0])
