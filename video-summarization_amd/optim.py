"""``Adam`` / ``AdamW`` — the parameter update of the training step on the MI355X-native kernel of
``include/vs_optim.h``: drop-ins for ``torch.optim.Adam`` (reference ``src/train.py:35``, ``src/pretrain.py:35``).

    optim = Adam(model.parameters(), lr=1e-5, weight_decay=1e-5)      # was: torch.optim.Adam(...)
    optim.attach(model)                                               # optional: write-through (below)

One HIP launch per 64 tensors updates ``p``, ``exp_avg`` and ``exp_avg_sq``.  An unmodified ``torch.amp.GradScaler``
drives it through its non-synchronising branch (``_step_supports_amp_scaling``): the scale and the overflow flag stay
device scalars, a step with an overflow leaves every tensor and the step count untouched, and the host is never asked.

Write-through: for the parameters of an attached ``SimNet`` (native shapes) whose packed weights are current, the same
launch stores the new values into the packed copy the kernels read, and the module's pack cache is told, so the next
forward does not re-pack (``vs_weights_update``).  Parameters of any other module go through the generic entry of the
same kernel; a ``SimNet`` that is not attached, is embedded in a wider shape, or whose cache is stale simply re-packs
on its next forward as it does after ``torch.optim.Adam``.

State lives under torch's own keys (``step`` - a device fp32 scalar, as torch's fused / capturable form keeps it -
``exp_avg``, ``exp_avg_sq``), so ``state_dict()`` loads into ``torch.optim.Adam`` and the other way round.  There is
no CPU path and no fallback to torch inside this class.

Clipping the global gradient norm: ``Adam(..., max_grad_norm=1.0)`` measures the norm of every gradient of the step on
the device (``vs_grad_norm_tensors``: squares summed in double) and hands ``grad_scale / clip_coef`` to the update kernel
as its divisor - one extra read of the gradients, no write, nothing read by the host.  ``clip_grad_norm_`` / ``grad_norm``
are the same kernels for a loop that keeps another optimizer.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional

import torch
from torch import Tensor, nn
from torch.optim import Optimizer

from . import _lib
from ._call import on_stream, ptr, scratch
from .simnet import SimNet

__all__ = ["Adam", "AdamW", "clip_grad_norm_", "grad_norm"]


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def _module_key(module: SimNet, device: torch.device):
    return (device,) + tuple((t.data_ptr(), t._version) for t in module._tensors())


def _check_max_norm(max_norm) -> float:
    if isinstance(max_norm, Tensor) or isinstance(max_norm, bool):
        raise ValueError("max_norm must be a Python float (it is passed to the kernel with the launch), got %r" % (type(max_norm).__name__,))
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("Invalid max_norm: %r (> 0; float('inf') measures without clipping)" % (max_norm,))
    return max_norm


def _norm_kind(norm_type) -> int:
    if not isinstance(norm_type, Tensor) and not isinstance(norm_type, (bool, str)):
        try:
            t = float(norm_type)
        except (TypeError, ValueError):
            t = None
        if t == 2.0:
            return _lib.VS_GRAD_NORM_L2
        if t == math.inf:
            return _lib.VS_GRAD_NORM_MAX
    raise ValueError("norm_type %r is not implemented by the HIP kernel: 2.0 or float('inf')" % (norm_type,))


class _ClipBuffers:
    """The persistent device buffers of a clipping optimizer: the four result scalars and the per-chunk partials."""

    def __init__(self, dev: torch.device):
        self.dev = dev
        self.out = torch.zeros((4,), dtype=torch.float32, device=dev)
        self.ws: Optional[Tensor] = None
        self.table = (_lib.GradTensor * 1)()

    def measure(self, lib, grads, kind: int, max_norm: float, grad_scale: Optional[Tensor], stream) -> Tensor:
        if len(grads) > len(self.table):
            self.table = (_lib.GradTensor * len(grads))()
        for e, g in zip(self.table, grads):
            e.g, e.n = g.data_ptr(), g.numel()
        need = lib.vs_grad_norm_workspace_bytes(self.table, len(grads))
        if need == 0:
            raise RuntimeError("a gradient has 2^32 elements or more")
        if self.ws is None or self.ws.numel() < need:
            self.ws = scratch(need, self.dev)
        _lib.check(lib.vs_grad_norm_tensors(self.table, len(grads), kind, max_norm, ptr(grad_scale),
                                            self.out.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream))
        return self.out


def _dense_grads(parameters, who: str):
    """the gradients of ``parameters`` for the free functions: HIP, fp32, dense, contiguous - or RuntimeError"""
    if isinstance(parameters, Tensor):
        parameters = [parameters]
    grads, dev = [], None
    for p in parameters:
        g = p.grad
        if g is None:
            continue
        if not p.is_cuda or not g.is_cuda:
            raise RuntimeError("%s runs on the MI355X HIP kernel only: parameter of shape %s is on %s (there is no CPU path; use "
                               "torch.nn.utils for CPU tensors)" % (who, tuple(p.shape), p.device))
        if g.is_sparse:
            raise RuntimeError("%s (HIP kernel) takes dense gradients, got a sparse one for a parameter of shape %s" % (who, tuple(p.shape)))
        if g.dtype != torch.float32:
            raise RuntimeError("%s (HIP kernel) takes fp32 gradients, got %s" % (who, g.dtype))
        if not g.is_contiguous():
            raise RuntimeError("%s (HIP kernel): the gradient of a parameter of shape %s is not contiguous - scaling a copy in place "
                               "would silently leave it unclipped; make it contiguous first" % (who, tuple(p.shape)))
        if dev is not None and g.device != dev:
            raise RuntimeError("%s: gradients on %s and %s - one global norm needs one device" % (who, dev, g.device))
        dev = g.device
        grads.append(g)
    return grads, dev


def _measure(parameters, max_norm: float, norm_type, who: str):
    kind = _norm_kind(norm_type)
    grads, dev = _dense_grads(parameters, who)
    if dev is None:
        return None, None, None
    lib = _lib.load()
    buf = _ClipBuffers(dev)
    with on_stream(dev) as stream:
        out = buf.measure(lib, grads, kind, max_norm, None, stream)
    return out, buf, len(grads)


@torch.no_grad()
def grad_norm(parameters, norm_type=2.0) -> Tensor:
    """``torch.nn.utils.get_total_norm`` of the gradients of ``parameters`` on the HIP kernel: the 0-dim fp32 device norm.
    Nothing is read by the host."""
    out, _, _ = _measure(parameters, math.inf, norm_type, "grad_norm")
    return torch.zeros(()) if out is None else out[0]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None) -> Tensor:
    """``torch.nn.utils.clip_grad_norm_`` on the HIP kernels: norm launches (squares summed in double), one finalize, one
    in-place scale that writes nothing when the norm is within ``max_norm``.  Returns the 0-dim fp32 device norm; the host
    reads nothing, which is why ``error_if_nonfinite=True`` is refused.  ``foreach`` is accepted and has no meaning here.
    With this library's ``Adam`` prefer ``Adam(max_grad_norm=...)``: it does not rewrite the gradients at all."""
    if error_if_nonfinite:
        raise ValueError("clip_grad_norm_(error_if_nonfinite=True) would read the norm on the host (a synchronisation): test the returned "
                         "device tensor yourself, or use torch.nn.utils.clip_grad_norm_")
    max_norm = _check_max_norm(max_norm)
    out, buf, n = _measure(parameters, max_norm, norm_type, "clip_grad_norm_")
    if out is None:
        return torch.zeros(())
    with on_stream(buf.dev) as stream:
        _lib.check(_lib.load().vs_grad_scale_tensors(buf.table, n, out.data_ptr() + 4, stream))
    return out[0]


class _ModulePart:
    """The parameters of ONE attached SimNet inside ONE param group: the structs ``vs_adam_step`` takes."""

    def __init__(self, module: SimNet, entries):
        L = module.num_layers
        self.module = module
        self.P, self.G = _lib.ModelParams(), _lib.ModelGrads()
        self._pl, self._gl = (_lib.LayerParams * max(L, 1))(), (_lib.LayerGrads * max(L, 1))()
        self.P.layers, self.G.layers = self._pl, self._gl
        pl, gl = [self._pl[l] for l in range(L)], [self._gl[l] for l in range(L)]
        self.slots = []         # (parameter, params struct, grads struct, field name)
        for p, idx in entries:
            if idx < 2:
                self.slots.append((p, self.P, self.G, ("embed_w", "embed_b")[idx]))
            elif idx >= 2 + 16 * L:
                self.slots.append((p, self.P, self.G, ("final_w", "final_b")[idx - 2 - 16 * L]))
            else:
                l, j = divmod(idx - 2, 16)
                self.slots.append((p, pl[l], gl[l], _lib._LAYER_FIELDS[j]))


class _GroupPlan:
    def __init__(self):
        self.key = None
        self.parts: List[_ModulePart] = []
        self.generic: List[Tensor] = []
        self.table = None           # (AdamTensor * len(generic))
        self.views: Dict[Tensor, tuple] = {}    # parameter -> (step, exp_avg, exp_avg_sq) views of the arenas
        self.keep = []              # the arenas
        self.live = set()           # id() of the parameters whose state is in Optimizer.state already
        self.dev = None


class Adam(Optimizer):
    """``torch.optim.Adam`` on the HIP multi-tensor kernel.  Same constructor; ``amsgrad``, ``maximize`` and
    ``differentiable`` are refused (not ignored); ``foreach`` / ``fused`` / ``capturable`` are accepted and have no
    meaning here (the step is always one fused launch, the step count always a device tensor).  ``model=``: see ``attach``.

    ``max_grad_norm`` (keyword only, default None: off) clips the global norm of ALL gradients of a step, across every
    param group, as ``torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm, grad_norm_type)`` before the
    step would - inside ``step()``, with or without a ``GradScaler`` (before or after ``unscale_``), without rewriting
    the gradients and without a host read.  ``grad_norm_type`` is 2.0 or ``inf``.  Both are attributes of the optimizer
    (``optim.max_grad_norm`` may be rewritten between steps) and are NOT part of ``defaults`` / ``param_groups``: the key
    set of ``state_dict()`` stays ``torch.optim.Adam``'s, so a checkpoint does not carry them - pass them again when the
    optimizer is rebuilt.  After a clipped step ``optim.last_grad_norm`` is the 0-dim device tensor of the measured norm
    (of the unscaled gradients), valid until the next step."""

    _step_supports_amp_scaling = True       # GradScaler.step: hand over grad_scale / found_inf, do not unscale or sync

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, model=None,
                 max_grad_norm=None, grad_norm_type=2.0):
        if amsgrad:
            raise ValueError("Adam(amsgrad=True) is not implemented by the HIP kernel (use torch.optim.Adam for it)")
        if maximize:
            raise ValueError("Adam(maximize=True) is not implemented by the HIP kernel (negate the loss instead)")
        if differentiable:
            raise ValueError("Adam(differentiable=True) is not implemented by the HIP kernel")
        if isinstance(lr, Tensor):
            raise ValueError("lr must be a Python float: it is passed to the kernel with every launch, a scheduler may rewrite it freely")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if max_grad_norm is not None:
            _check_max_norm(max_grad_norm)
        _norm_kind(grad_norm_type)
        # the key set of torch.optim.Adam's groups, so a state_dict moves between the two classes
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=foreach,
                        capturable=True, differentiable=False, fused=fused, decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults)
        self._modules: List[SimNet] = []
        self._plans: Dict[int, _GroupPlan] = {}
        self._module_state: Dict[SimNet, Tensor] = {}     # one vs_adam_state buffer per attached module
        self._sync_word: Optional[Tensor] = None
        self.max_grad_norm = max_grad_norm
        self.grad_norm_type = grad_norm_type
        self.last_grad_norm: Optional[Tensor] = None
        self._clip: Optional[_ClipBuffers] = None
        if model is not None:
            self.attach(model)

    # ---- write-through ------------------------------------------------------------------------
    def attach(self, model: nn.Module) -> "Adam":
        """Links every ``SimNet`` inside ``model`` (the model itself, ``PretrainModel.encoder``, ...) for write-through.
        Optional: without it every step is still correct, the next forward re-packs as after torch's Adam."""
        for m in model.modules():
            if isinstance(m, SimNet) and m not in self._modules:
                self._modules.append(m)
        self._plans.clear()
        return self

    def __setstate__(self, state):          # unpickled: Optimizer keeps defaults / state / param_groups only
        super().__setstate__(state)
        self.__dict__.setdefault("_modules", [])
        self.__dict__.setdefault("_module_state", {})
        self.__dict__.setdefault("_sync_word", None)
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("grad_norm_type", 2.0)
        self.__dict__.setdefault("last_grad_norm", None)
        self._clip = None
        self._plans = {}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans.clear()         # the loaded tensors are moved into the arenas by the next step

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_plans"):
            self._plans.clear()

    # ---- plans: built on the first step of a group, rebuilt when its parameter list changes --------
    def _device_of(self, group) -> torch.device:
        dev = None
        for p in group["params"]:
            if not p.is_cuda:
                raise RuntimeError("Adam runs on the MI355X HIP kernel only: parameter of shape %s is on %s - move the model to a "
                                   "HIP device (there is no CPU path and no fallback to torch.optim.Adam)" % (tuple(p.shape), p.device))
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("Adam (HIP kernel) takes contiguous fp32 parameters, got %s%s" % (p.dtype, "" if p.is_contiguous() else " (strided)"))
            if dev is not None and p.device != dev:
                raise RuntimeError("Adam (HIP kernel): the parameters of one group are on %s and %s" % (dev, p.device))
            dev = p.device
        return dev

    def _build_plan(self, gi: int, group, dev: torch.device) -> _GroupPlan:
        lib = _lib.load()
        plan = _GroupPlan()
        plan.key = tuple(id(p) for p in group["params"])
        old = {p: {k: v.detach().clone() for k, v in self.state[p].items()} for p in group["params"] if len(self.state.get(p, ())) > 0}
        in_group = {id(p) for p in group["params"]}
        taken = set()
        for module in self._modules:
            if module._plan is not None or module._plan_error is not None or module._packed is None or module._packed.device != dev:
                continue            # embedded shapes and modules that never ran: generic entry + the module's own re-pack
            entries, idx = [], 0
            for t in module._tensors():
                if not isinstance(t, nn.Parameter):
                    continue        # the positional table: a buffer
                if id(t) in in_group and id(t) not in taken and t.dtype == torch.float32 and t.is_contiguous():
                    entries.append((t, idx))
                idx += 1
            if not entries:
                continue
            handle = module._packed.handle
            buf = self._module_state.get(module)
            if buf is None or buf.device != dev:
                buf = torch.zeros((lib.vs_adam_state_bytes(handle),), dtype=torch.uint8, device=dev)
                self._module_state[module] = buf
            off, cnt = C.c_size_t(), C.c_size_t()
            for p, i in entries:
                v3 = []
                for which in (2, 0, 1):
                    _lib.check(lib.vs_adam_state_field(handle, i, which, C.byref(off), C.byref(cnt)))
                    if which != 2 and cnt.value != p.numel():
                        raise RuntimeError("parameter %d of the attached SimNet has %d elements, the packed model %d" % (i, p.numel(), cnt.value))
                    v = buf[off.value: off.value + 4 * cnt.value].view(torch.float32)
                    v3.append(v.view(()) if which == 2 else v.view(p.shape))
                plan.views[p] = tuple(v3)
                taken.add(id(p))
            plan.parts.append(_ModulePart(module, entries))
        plan.generic = [p for p in group["params"] if id(p) not in taken]
        if plan.generic:
            offs = [0]
            for p in plan.generic:
                offs.append(offs[-1] + _pad64(p.numel()))
            m_arena = torch.zeros((offs[-1],), dtype=torch.float32, device=dev)
            v_arena = torch.zeros((offs[-1],), dtype=torch.float32, device=dev)
            steps = torch.zeros((len(plan.generic),), dtype=torch.float32, device=dev)
            plan.keep = [m_arena, v_arena, steps]
            plan.table = (_lib.AdamTensor * len(plan.generic))()
            for i, p in enumerate(plan.generic):
                n = p.numel()
                m, v, s = m_arena[offs[i]: offs[i] + n].view(p.shape), v_arena[offs[i]: offs[i] + n].view(p.shape), steps[i]
                plan.views[p] = (s, m, v)
                e = plan.table[i]
                e.m, e.v, e.step, e.mirror = m.data_ptr(), v.data_ptr(), s.data_ptr(), None
        # state that exists already (a loaded checkpoint, an earlier plan) moves into the views
        for p, (s, m, v) in plan.views.items():
            st = old.get(p)
            if st is None:
                s.zero_(); m.zero_(); v.zero_()
                continue
            s.copy_(torch.as_tensor(st["step"], dtype=torch.float32).reshape(()))
            m.copy_(st["exp_avg"]); v.copy_(st["exp_avg_sq"])
            self.state[p] = {"step": s, "exp_avg": m, "exp_avg_sq": v}
            plan.live.add(id(p))
        return plan

    def _plan_of(self, gi: int, group) -> _GroupPlan:
        plan = self._plans.get(gi)
        if plan is None or plan.key != tuple(id(p) for p in group["params"]):
            dev = self._device_of(group)          # every parameter: HIP device, fp32, contiguous (raises otherwise)
            with torch.cuda.device(dev):
                plan = self._plans[gi] = self._build_plan(gi, group, dev)
            plan.dev = dev
        return plan

    # ---- clipping: the norm of every gradient of the step, and the divisor the update kernel takes ------------------
    def _clip_divisor(self, lib, grad_scale, pre) -> int:
        """Issues the norm launches over the gradients of ALL groups and returns the device address of
        ``grad_scale / clip_coef``.  ``pre``: id(parameter) -> the (contiguous) gradient the step will read."""
        max_norm = _check_max_norm(self.max_grad_norm)
        kind = _norm_kind(self.grad_norm_type)
        dev, grads = None, []
        for gi, group in enumerate(self.param_groups):
            if not group["params"]:
                continue
            plan = self._plan_of(gi, group)
            if dev is not None and plan.dev != dev:
                raise RuntimeError("Adam(max_grad_norm=...): the param groups are on %s and %s - one global norm needs one device"
                                   % (dev, plan.dev))
            dev = plan.dev
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda or p.dtype is not torch.float32:
                    self._device_of(group)              # moved or cast since the plan was built: raises with the reason
                if g.is_sparse:
                    raise RuntimeError("Adam (HIP kernel) takes dense gradients, got a sparse one for a parameter of shape %s" % (tuple(p.shape),))
                if not g.is_contiguous():
                    g = g.contiguous()
                pre[id(p)] = g
                grads.append(g)
        if dev is None:
            raise RuntimeError("Adam(max_grad_norm=...): the optimizer has no parameters")
        if grad_scale is not None and (grad_scale.device != dev or grad_scale.dtype != torch.float32):
            raise RuntimeError("grad_scale / found_inf must be fp32 scalars on %s, got %s on %s" % (dev, grad_scale.dtype, grad_scale.device))
        if self._clip is None or self._clip.dev != dev:
            self._clip = _ClipBuffers(dev)
        with on_stream(dev) as stream:
            out = self._clip.measure(lib, grads, kind, max_norm, grad_scale, stream)
        self.last_grad_norm = out[0]
        return out.data_ptr() + 8

    # ---- the step -----------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        grad_scale = getattr(self, "grad_scale", None)       # set by torch.amp.GradScaler.step for the call
        found_inf = getattr(self, "found_inf", None)
        current = {}            # attached module -> its pack-cache key if the cache is current (write-through), else None
        touched = []
        pre = {}                # clipping: id(parameter) -> the gradient that was measured (the one the kernel then reads)
        divisor = self._clip_divisor(lib, grad_scale, pre) if self.max_grad_norm is not None else None
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            plan = self._plan_of(gi, group)
            dev = plan.dev
            for t in (grad_scale, found_inf):
                if t is not None and (t.device != dev or t.dtype != torch.float32):
                    raise RuntimeError("grad_scale / found_inf must be fp32 scalars on %s, got %s on %s" % (dev, t.dtype, t.device))
            beta1, beta2 = group["betas"]
            cfg = _lib.AdamCfg(float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                               1 if group.get("decoupled_weight_decay", False) else 0, 0)
            gs, fi = ptr(grad_scale), ptr(found_inf)
            if divisor is not None:
                gs = divisor        # grad_scale / clip_coef: the kernel's division unscales and clips at once
            state, views, live, hold, f32 = self.state, plan.views, plan.live, [], torch.float32

            def grad_ptr(p):
                # (torch itself refuses a .grad whose dtype, device or shape differs from its parameter's)
                g = p.grad
                if g is None:
                    return None
                if id(p) in pre:
                    g = pre[id(p)]                      # checked (and made contiguous) when the norm was measured
                else:
                    if not p.is_cuda or p.dtype is not f32:
                        self._device_of(group)              # moved or cast since the plan was built: raises with the reason
                    if g.is_sparse:
                        raise RuntimeError("Adam (HIP kernel) takes dense gradients, got a sparse one for a parameter of shape %s" % (tuple(p.shape),))
                    if not g.is_contiguous():
                        g = g.contiguous()
                        hold.append(g)
                if id(p) not in live:           # first gradient of this parameter: its state becomes visible, as in torch
                    s, m, v = views[p]
                    state[p] = {"step": s, "exp_avg": m, "exp_avg_sq": v}
                    live.add(id(p))
                touched.append(p)
                return g.data_ptr()

            with on_stream(dev) as stream:
                for part in plan.parts:
                    module = part.module
                    if module not in current:
                        packed = module._packed
                        key = _module_key(module, dev) if packed is not None and packed.device == dev else None
                        current[module] = key if (key is not None and key == module._packed_key) else None
                    through = current[module] is not None
                    if through:
                        any_grad = False
                        for p, ps, gs_, name in part.slots:
                            gp = grad_ptr(p)
                            setattr(gs_, name, gp)
                            setattr(ps, name, p.data_ptr())
                            any_grad |= gp is not None
                        if any_grad:
                            _lib.check(lib.vs_adam_step(module._packed.handle, C.byref(part.P), C.byref(part.G),
                                                        self._module_state[module].data_ptr(), C.byref(cfg), gs, fi, stream))
                    else:           # stale or missing pack cache: same kernel without the mirror, the module re-packs itself
                        tab = (_lib.AdamTensor * len(part.slots))()
                        for e, (p, _, _, _) in zip(tab, part.slots):
                            s, m, v = views[p]
                            gp = grad_ptr(p)
                            e.p, e.g, e.m, e.v, e.step, e.n = p.data_ptr(), gp, m.data_ptr(), v.data_ptr(), s.data_ptr(), (p.numel() if gp else 0)
                        _lib.check(lib.vs_adam_step_tensors(tab, len(tab), C.byref(cfg), gs, fi, self._sync(dev).data_ptr(), stream))
                if plan.generic:
                    for e, p in zip(plan.table, plan.generic):
                        gp = grad_ptr(p)
                        e.p, e.g, e.n = p.data_ptr(), gp, (p.numel() if gp else 0)
                    _lib.check(lib.vs_adam_step_tensors(plan.table, len(plan.generic), C.byref(cfg), gs, fi,
                                                        self._sync(dev).data_ptr(), stream))
            del hold
        if touched:
            torch._C._increment_version(touched)      # the kernel wrote through raw pointers: tell autograd / the pack caches
        for module, key in current.items():
            if key is not None:
                # the packed copy holds the new values already: the cache stays current, the next forward does not re-pack
                module._packed_key = _module_key(module, key[0])
        return loss

    def _sync(self, dev: torch.device) -> Tensor:
        if self._sync_word is None or self._sync_word.device != dev:
            self._sync_word = torch.zeros((64,), dtype=torch.int32, device=dev)
        return self._sync_word


class AdamW(Adam):
    """``torch.optim.AdamW``: decoupled weight decay (``p *= 1 - lr * weight_decay`` before the update), default 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, model=None, max_grad_norm=None,
                 grad_norm_type=2.0):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True, model=model,
                         max_grad_norm=max_grad_norm, grad_norm_type=grad_norm_type)
