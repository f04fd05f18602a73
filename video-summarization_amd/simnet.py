"""``SimNet`` — drop-in for the reference frame-importance scorer, MI355X-native.

Same constructor, ``forward`` signature/return tuple and ``state_dict`` key set as the reference
``model.SimNet`` (reference ``src/model/simnet.py:8-56``; key list SURVEY.md §8(a) row 1), so
``src/train.py``, ``src/pretrain.py``, ``src/evaluation`` and ``PretrainModel`` call it unchanged
and reference checkpoints load ``strict=True``.

Scoring (eval / no-grad) runs entirely in the hand-written gfx950 kernels of ``libvsscore.so``
through the custom op ``vs_amd::score_frames``; calls that need autograd (``train.py:121``,
``pretrain.py:61``: train mode, dropout, backward) run ``_TrainForward``, a ``torch.autograd.Function``
over the training C ABI (``include/vs_train.h``): HIP forward that keeps its activations, HIP backward
(flash-attention backward, dgrad / wgrad GEMMs, LayerNorm / ReLU / dropout backward).  There is NO PyTorch
or CPU fallback for either: a missing library or a non-HIP tensor raises.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from ._call import host_lengths, mask_u8, on_stream, ptr, scratch
from .synth import IN_FEATURES, PE_MAX_LEN, positional_table

# --------------------------------------------------------------------------------------------
# packed-weight handles (vs_weights*) live in a registry so the custom op can take a plain int
# --------------------------------------------------------------------------------------------


class _Packed:
    """Owns one ``vs_weights*`` (device copy of the parameters in kernel layout)."""

    def __init__(self, handle: int, device: torch.device):
        self.handle = handle
        self.device = device

    def __del__(self):
        try:
            if self.handle:
                _lib.load().vs_weights_free(self.handle)
                self.handle = 0
        except Exception:
            pass


@torch.library.custom_op("vs_amd::score_frames", mutates_args=(), device_types="cuda")
def score_frames(x: Tensor, mask: Optional[Tensor], handle: int, d_model: int, num_classes: int,
                 flags: int, want_hidden: bool) -> Tuple[Tensor, Tensor]:
    """x [B,T,Din] fp32 (HIP device), mask bool/uint8 [B,T] or None, handle = vs_weights*.
    Returns (scores [B,T,num_classes], hidden [B,T,d_model] or an empty tensor)."""
    lib = _lib.load()
    B, T, _ = x.shape
    x = x.contiguous()
    scores = torch.empty((B, T, num_classes), dtype=torch.float32, device=x.device)
    hidden = torch.empty((B, T, d_model) if want_hidden else (0,), dtype=torch.float32, device=x.device)
    m = mask_u8(mask)
    with on_stream(x.device) as stream:
        ws = scratch(lib.vs_scorer_workspace_bytes(handle, B, T), x.device, floor=256)
        _lib.check(lib.vs_scorer_forward(handle, x.data_ptr(), ptr(m), B, T, flags, scores.data_ptr(),
                                         hidden.data_ptr() if want_hidden else None, ws.data_ptr(),
                                         ws.numel(), stream))
    return scores, hidden


@score_frames.register_fake
def _(x, mask, handle, d_model, num_classes, flags, want_hidden):
    B, T, _ = x.shape
    return (x.new_empty((B, T, num_classes), dtype=torch.float32),
            x.new_empty((B, T, d_model) if want_hidden else (0,), dtype=torch.float32))


def score_frames_packed(x: Tensor, lengths, handle: int, d_model: int, num_classes: int, flags: int,
                        want_hidden: bool) -> Tuple[Tensor, Tensor]:
    """Packed ragged batch: x [sum(lengths), Din] fp32 (HIP device) = the frames of len(lengths) videos concatenated.
    Returns (scores [Mtot, num_classes], hidden [Mtot, d_model] or an empty tensor).  No padding, no mask."""
    lib = _lib.load()
    lengths, host = host_lengths(lengths)
    if x.dim() != 2 or x.size(0) != sum(lengths):
        raise RuntimeError("expected x of shape [sum(lengths)=%d, D], got %s" % (sum(lengths), tuple(x.shape)))
    x = x.contiguous()
    M, B = x.size(0), len(lengths)
    scores = torch.empty((M, num_classes), dtype=torch.float32, device=x.device)
    hidden = torch.empty((M, d_model) if want_hidden else (0,), dtype=torch.float32, device=x.device)
    with on_stream(x.device) as stream:
        dev_len = torch.tensor(lengths, dtype=torch.int32, device=x.device)
        need = lib.vs_scorer_workspace_bytes_packed(handle, host, B)
        if need == 0:
            _lib.check(lib.vs_scorer_forward_packed(handle, x.data_ptr(), host, dev_len.data_ptr(), B, flags,
                                                    scores.data_ptr(), None, None, 0, None))   # raises with the reason
        ws = scratch(need, x.device)
        _lib.check(lib.vs_scorer_forward_packed(handle, x.data_ptr(), host, dev_len.data_ptr(), B, flags,
                                                scores.data_ptr(), hidden.data_ptr() if want_hidden else None,
                                                ws.data_ptr(), ws.numel(), stream))
    return scores, hidden


# --------------------------------------------------------------------------------------------
# training path: torch.autograd.Function over include/vs_train.h
# --------------------------------------------------------------------------------------------


class _TrainBatch(NamedTuple):
    """How one training batch is described to include/vs_train.h, and the four entry points that take that description:
    ``sizes`` follow the weights in the two size queries, ``where`` stands between ``x`` and the dropout config in the forward
    and the backward.  Padded: (B, T) and (mask, B, T); packed: (lengths, n) and (lengths, lengths_dev, n)."""
    sizes: tuple
    where: tuple
    frames: int
    saved_bytes: object
    workspace_bytes: object
    forward: object
    backward: object


def _train_batch(lib, x: Tensor, keep: Optional[Tensor], lengths) -> _TrainBatch:
    """``lengths`` None: x [B, T, in] with ``keep`` its uint8 mask (or None); else x [sum(lengths), in] with ``keep`` the
    lengths on the device.  ``keep`` is what the Function saves beside ``x``: ``where`` holds its address."""
    if lengths is None:
        B, T, _ = x.shape
        return _TrainBatch((B, T), (ptr(keep), B, T), B * T, lib.vs_train_saved_bytes, lib.vs_train_workspace_bytes,
                           lib.vs_train_forward, lib.vs_train_backward)
    lengths, host = host_lengths(lengths)
    return _TrainBatch((host, len(lengths)), (host, keep.data_ptr(), len(lengths)), x.size(0), lib.vs_train_saved_bytes_packed,
                       lib.vs_train_workspace_bytes_packed, lib.vs_train_forward_packed, lib.vs_train_backward_packed)


class _TrainForward(torch.autograd.Function):
    """``SimNet.forward`` (reference train.py:121 / pretrain.py:61) and ``SimNet.forward_packed_train`` under autograd: forward
    and backward are the HIP kernels behind ``vs_train_forward`` / ``vs_train_backward``, or behind their ``_packed`` forms on
    the frames of several videos concatenated (``lengths`` given: no sentinel rows, no mask, nothing computed for padding).
    The parameters are passed as inputs so autograd routes their gradients; the activation record is one uint8 tensor
    saved for the backward."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)     # train.py:120 calls under amp.autocast()
    def forward(ctx, module, x, mask, lengths, p, p_embed, seed, tflags, *params):
        lib = _lib.load()
        x = x.contiguous()
        packed = module._packed_weights(x.device)
        scores = torch.empty(x.shape[:-1] + (module.num_classes,), dtype=torch.float32, device=x.device)
        hidden = torch.empty(x.shape[:-1] + (module._lib_d,), dtype=torch.float32, device=x.device)
        cfg = _lib.DropoutCfg(float(p_embed), float(p), int(seed), int(tflags), 0)
        with on_stream(x.device) as stream:
            if not getattr(packed, "train_prepared", False):     # one-time allocation of the dgrad transposes, outside the backward
                _lib.check(lib.vs_train_prepare(packed.handle, stream))
                packed.train_prepared = True
            keep = mask_u8(mask) if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=x.device)
            batch = _train_batch(lib, x, keep, lengths)
            need = batch.saved_bytes(packed.handle, *batch.sizes)
            # *batch.where below: (mask, B, T) of vs_train_forward, (lengths, lengths_dev, n) of vs_train_forward_packed
            if need == 0 and lengths is not None:       # invalid lengths: the forward says why
                _lib.check(batch.forward(packed.handle, x.data_ptr(), *batch.where, C.byref(cfg), scores.data_ptr(), None, None, 0,
                                         None, 0, stream))
            saved = scratch(need, x.device)
            ws = scratch(batch.workspace_bytes(packed.handle, *batch.sizes), x.device)
            _lib.check(batch.forward(packed.handle, x.data_ptr(), *batch.where, C.byref(cfg), scores.data_ptr(), hidden.data_ptr(),
                                     saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(), stream))
            fmt = int(lib.vs_train_last_format())        # the form this record was written in: handed back to the backward
        ctx.save_for_backward(x, keep, saved)
        ctx.module, ctx.cfg, ctx.packed, ctx.packed_key = module, (float(p_embed), float(p), int(seed), int(tflags), fmt), packed, module._packed_key
        ctx.lengths = None if lengths is None else tuple(lengths)
        if lengths is None:
            module._note_train_arithmetic(int(tflags), fmt, batch.frames)
        else:       # (last_train_dtype names the Linears' arithmetic; the packed attention has a word of its own)
            module._note_train_arithmetic(int(tflags) & ~(_lib.VS_TRAIN_FLAG_BF16_ATTENTION | _lib.VS_TRAIN_FLAG_PACKED_LP_ATTENTION), fmt, batch.frames)
            form = _lib.train_form(fmt)
            module._last_packed_attention_dtype = form.dtype(form.lpa)
        ctx.set_materialize_grads(False)
        return scores, (hidden[..., :module.d_model] if module._plan else hidden)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_scores, d_hidden):
        lib = _lib.load()
        x, keep, saved = ctx.saved_tensors
        module, packed = ctx.module, ctx.packed
        if module._packed_key != ctx.packed_key or module._packed is not packed:
            raise RuntimeError("SimNet parameters were modified between forward and backward")
        batch = _train_batch(lib, x, keep, ctx.lengths)
        grads, G, finish = _grad_destinations(module, x.device)
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        ds = None if d_scores is None else d_scores.contiguous().float()
        dh = None if d_hidden is None else d_hidden.contiguous().float()
        if dh is not None and module._plan:
            dh = module._pad(dh, ("res",)).contiguous()
        cfg = _lib.DropoutCfg(*ctx.cfg)
        with on_stream(x.device) as stream:
            ws = scratch(batch.workspace_bytes(packed.handle, *batch.sizes), x.device)
            # *batch.where: (mask, B, T) of vs_train_backward, (lengths, lengths_dev, n) of vs_train_backward_packed
            _lib.check(batch.backward(packed.handle, x.data_ptr(), *batch.where, C.byref(cfg), ptr(ds), ptr(dh), saved.data_ptr(),
                                      saved.numel(), C.byref(G), ptr(dx), ws.data_ptr(), ws.numel(), stream))
        return (None, dx, None, None, None, None, None, None, *finish(grads))


def _model_struct(cls, tensors, num_layers: int, use_pos: bool = False):
    """A ``vs_model_params`` / ``vs_model_grads`` (``cls``) whose fields point at ``tensors``, given in the order of
    ``SimNet._tensors()`` (``use_pos``: with the positional table, which only the parameters have)."""
    it = iter(tensors)
    S = cls()
    S.embed_w, S.embed_b = next(it).data_ptr(), next(it).data_ptr()
    if use_pos:
        S.pos_embedding = next(it).data_ptr()
    layers = (_lib.LayerParams * max(num_layers, 1))()
    for l in range(num_layers):
        for name in _lib._LAYER_FIELDS:
            setattr(layers[l], name, next(it).data_ptr())
    S.layers = layers
    S.final_w, S.final_b = next(it).data_ptr(), next(it).data_ptr()
    return S


def _grad_destinations(module, device):
    """The gradient tensors of one backward and the ``vs_model_grads`` that points at them: ONE allocation, viewed per
    parameter (was ~70 torch.empty_like per backward).  Returns (grads, G, finish); ``finish(grads)`` gives autograd's
    per-parameter return values (true shapes of an embedded model, None where no gradient is required)."""
    params = [t for t in module._tensors() if isinstance(t, nn.Parameter)]
    axes = [ax for t, ax in zip(module._tensors(), module._tensor_axes()) if isinstance(t, nn.Parameter)]
    shapes = [t.shape for t in params]
    if module._plan:      # embedded model: the library writes gradients of ITS shape; the true-shaped parts go back
        shapes = [module._padded_shape(t.shape, ax) for t, ax in zip(params, axes)]
    sizes = [int(torch.Size(sh).numel()) for sh in shapes]
    if all(n_ % 4 == 0 for n_ in sizes[:-1]):
        # dense packing keeps every view 16-byte aligned (all the kernels need); the views come from ONE C++ call
        flat = torch.empty((sum(sizes),), dtype=torch.float32, device=device)
        grads = [g.view(sh) for g, sh in zip(flat.split_with_sizes(sizes), shapes)]
    else:
        offs = [0]
        for n_ in sizes:
            offs.append(offs[-1] + (n_ + 63) // 64 * 64)          # 256-byte aligned views
        flat = torch.empty((offs[-1],), dtype=torch.float32, device=device)
        grads = [flat[o: o + n_].view(sh) for o, n_, sh in zip(offs, sizes, shapes)]
    G = _model_struct(_lib.ModelGrads, grads, module.num_layers)

    def finish(gs):
        if module._plan:
            gs = [module._unpad(g, ax).contiguous() for g, ax in zip(gs, axes)]
        return [g if t.requires_grad else None for g, t in zip(gs, params)]
    return grads, G, finish


# --------------------------------------------------------------------------------------------
# shapes outside the kernels' envelope: the model EMBEDDED in the next supported shape (include/vs_scorer.h,
# vs_weights_set_norm_width)
# --------------------------------------------------------------------------------------------


# the head dims each low-precision attention arithmetic has kernels for (the library's, not the model's, when it is embedded):
# 'bf16' / 'fp16x3' of scoring (set_compute_dtype), 'bf16' / 'fp16' of packed training (set_train_dtype(..., packed_attention=True));
# the exact fp32 attention takes every head dim of embedding_plan
_ATTENTION_HEAD_DIMS = {"bf16": (32, 64, 128), "fp16x3": (32, 64), "fp16": (32, 64, 128)}


def embedding_plan(d_model: int, num_heads: int) -> Optional[Tuple[int, int]]:
    """The reference accepts any ``d_model % num_heads == 0`` (simnet.py:123); the kernels take d_model % 64 == 0 (<= 1024)
    with head dim 32 / 64 / 128 (/ 256: exact attention only, a correctness-first kernel).  Returns None for such a shape, else ``(d_lib, dh_lib)``: the narrowest supported shape
    with the same number of heads that holds the model when its parameters are zero-padded - mathematically the same
    function once LayerNorm and the attention scale use the true d_model, which the library is told
    (``vs_weights_set_norm_width``)."""
    dh = d_model // num_heads
    if d_model % 64 == 0 and d_model <= 1024 and dh in (32, 64, 128, 256):
        return None
    if d_model % 4 == 0:
        for dhp in (32, 64, 128, 256):
            if dhp >= dh and (num_heads * dhp) % 64 == 0 and num_heads * dhp <= 1024:
                return num_heads * dhp, dhp
    raise NotImplementedError("SimNet(d_model=%d, num_heads=%d): supported are d_model %% 4 == 0 with head dim <= 256 and "
                              "num_heads * (head dim rounded up to 32 / 64 / 128 / 256) <= 1024" % (d_model, num_heads))


# --------------------------------------------------------------------------------------------
# parameter containers: only there to give the state_dict its reference key names
# --------------------------------------------------------------------------------------------


class _Bag(nn.Module):
    """A named group of sub-modules / buffers with no behaviour of its own."""

    def __init__(self, **children):
        super().__init__()
        for name, child in children.items():
            setattr(self, name, child)


class _SinusoidTable(nn.Module):
    def __init__(self, d_model: int, max_len: int):
        super().__init__()
        self.register_buffer("pos_embedding", positional_table(d_model, max_len))


def _encoder_block(d: int) -> nn.Module:
    return _Bag(
        sa=_Bag(q=nn.Linear(d, d), k=nn.Linear(d, d), v=nn.Linear(d, d), feature_projection=nn.Linear(d, d)),
        mlp=_Bag(fc1=nn.Linear(d, 4 * d), fc2=nn.Linear(4 * d, d)),
        norm1=nn.LayerNorm(d), norm2=nn.LayerNorm(d))


class SimNet(nn.Module):
    """Transformer-encoder frame scorer: features [B,T,1024] -> (logits [B,T,num_classes], hidden [B,T,d])."""

    def __init__(self, num_heads: int = 8, d_model: int = 512, num_layers: int = 4,
                 sparsity: float = 0.5, use_cls: bool = False, dropout: float = 0.2,
                 num_classes: int = 1, use_pos: bool = True, max_len=2500, *,
                 in_features: int = IN_FEATURES, pe_len: int = PE_MAX_LEN):
        """Positional arguments are the reference's (simnet.py:10-13).  Keyword-only extensions, both
        defaulting to the reference's hard-coded values: ``in_features`` (simnet.py:22: 1024) and ``pe_len``
        (rows of the positional table, simnet.py:188: 2000) — BASELINE configs[4] (T=8192, 2048-d CLIP
        features) needs both; the oracle for it is the re-parameterised restatement."""
        super().__init__()
        if d_model % num_heads:
            raise AssertionError("d_model must be divisible by num_heads")      # simnet.py:123
        self.num_heads, self.d_model, self.num_layers = num_heads, d_model, num_layers
        self.sparsity, self.use_cls, self.max_len = sparsity, use_cls, max_len
        self.num_classes, self.in_features = num_classes, in_features            # simnet.py:22
        self.pe_len = pe_len
        self.use_pos, self.drop_rate = use_pos, dropout
        # the shape the kernels run: the model's own, or the supported shape it is embedded in (zero-padded parameters)
        # (a shape that fits neither still constructs - its state_dict is the reference's - and raises when it is run)
        self._plan_error = None
        try:
            self._plan = embedding_plan(d_model, num_heads)
        except NotImplementedError as exc:
            self._plan, self._plan_error = None, exc
        self._lib_d = self._plan[0] if self._plan else d_model
        self._lib_dh = self._plan[1] if self._plan else d_model // num_heads
        self._pad_index = {}              # device -> index vectors of the padding maps

        emb = dict(feature_transform=nn.Linear(self.in_features, d_model))
        if use_pos:
            emb["positional_encoding"] = _SinusoidTable(d_model, pe_len)        # simnet.py:188 (2000, not max_len)
        self.embedding_layer = _Bag(**emb)
        if use_cls:
            # simnet.py:205-206: a learnable token prepended AFTER the positional encoding (:214-216); a direct
            # parameter of the embedding module, so it comes first in the state_dict like the reference's
            self.embedding_layer.cls_token = nn.Parameter(torch.zeros((1, 1, d_model)))
        self.encoder = _Bag(module_list=nn.ModuleList(_encoder_block(d_model) for _ in range(num_layers)),
                            module_score=nn.ModuleList())                        # stays empty: SURVEY Q2
        self.final_layer = nn.Linear(d_model, num_classes)
        self.fused_sigmoid = False        # opt-in: fold the callers' torch.sigmoid (train.py:144) into the kernel
        # opt-in, long videos (BASELINE config 5): "bf16" runs the two attention products on the bf16 matrix
        # pipe (fp32 softmax/accumulation); scores then differ from the fp32 reference by ~1e-3, so the
        # default "fp32" is the only mode the 1e-4 parity bar applies to.
        self._attention_dtype = "fp32"
        self._linear_dtype = "fp32"       # "bf16": every Linear multiplies bf16-rounded operands (fp32 storage/accumulate)
        self.latency_mode = False         # opt-in (set_latency_mode): split-K kernels for one reference-sized video per call
        self._train_dtype = "fp32"        # set_train_dtype("bf16"): the training path's counterpart of the reference's autocast
        self.last_train_dtype = None      # what the last training forward actually computed in ("fp32" / "bf16" / "fp16")
        self._packed_attention = False    # set_train_dtype(..., packed_attention=True): packed batches' attention on the 16-bit pipe too
        self._last_packed_attention_dtype = "fp32"
        self._packed: Optional[_Packed] = None
        self._packed_key = None
        self._packed_shape = None
        self._packed_pe_key = None

    # ---- reference helper kept for API parity (simnet.py:47-56) ----
    def process_mask(self, mask: Tensor) -> Tensor:
        if self.use_cls:                                     # simnet.py:48-51: the class token is never padding
            mask = torch.cat([torch.zeros((mask.size(0), 1), dtype=mask.dtype, device=mask.device), mask], dim=1)
        B, N = mask.size()
        return mask.view(B, 1, 1, N).expand(B, self.num_heads, N, N)

    # ---- weight packing -------------------------------------------------------------------
    def _tensors(self):
        yield self.embedding_layer.feature_transform.weight
        yield self.embedding_layer.feature_transform.bias
        if self.use_pos:
            yield self.embedding_layer.positional_encoding.pos_embedding
        for blk in self.encoder.module_list:
            for lin in (blk.sa.q, blk.sa.k, blk.sa.v, blk.sa.feature_projection):
                yield lin.weight
                yield lin.bias
            yield blk.norm1.weight
            yield blk.norm1.bias
            yield blk.mlp.fc1.weight
            yield blk.mlp.fc1.bias
            yield blk.mlp.fc2.weight
            yield blk.mlp.fc2.bias
            yield blk.norm2.weight
            yield blk.norm2.bias
        yield self.final_layer.weight
        yield self.final_layer.bias

    # ---- embedding in a supported shape (self._plan) -----------------------------------------
    def _tensor_axes(self):
        """(rows, cols) axis kinds of every tensor of ``_tensors()``: 'res' residual-stream feature c -> c, 'head' feature
        (h, j) -> h * dh_lib + j, 'hid' the MLP's hidden axis (c -> c of 4 d_lib), None an axis that is not padded."""
        yield ("res", None)                                   # embed_w [d, in]
        yield ("res",)                                        # embed_b
        if self.use_pos:
            yield (None, "res")                               # pos_embedding [.., L, d]: last axis
        for _ in range(self.num_layers):
            for _qkv in range(3):
                yield ("head", "res")
                yield ("head",)
            yield ("res", "head")                             # feature_projection [d, d]
            yield ("res",)
            yield ("res",)
            yield ("res",)                                    # norm1
            yield ("hid", "res")
            yield ("hid",)                                    # fc1
            yield ("res", "hid")
            yield ("res",)                                    # fc2
            yield ("res",)
            yield ("res",)                                    # norm2
        yield (None, "res")                                   # final_layer.weight [nc, d]
        yield (None,)                                         # final_layer.bias

    def _axis(self, kind: Optional[str], device: torch.device):
        """(index vector of the true features inside the padded axis, padded length) - None for an unpadded axis"""
        if kind is None:
            return None
        tab = self._pad_index.get(device)
        if tab is None:
            d, H = self.d_model, self.num_heads
            c = torch.arange(d, device=device)
            tab = {"res": (c, self._lib_d), "head": ((c // (d // H)) * self._lib_dh + c % (d // H), self._lib_d),
                   "hid": (torch.arange(4 * d, device=device), 4 * self._lib_d)}
            self._pad_index[device] = tab
        return tab[kind]

    def _padded_shape(self, shape, axes):
        size = {"res": self._lib_d, "head": self._lib_d, "hid": 4 * self._lib_d}
        tail = tuple(size[k] if k else n for n, k in zip(shape[len(shape) - len(axes):], axes))
        return tuple(shape[:len(shape) - len(axes)]) + tail

    def _pad(self, t: Tensor, axes) -> Tensor:
        """t (true shape) -> zero-padded tensor of the library's shape; the last len(axes) dims are mapped"""
        if len(axes) == 1:
            ax = self._axis(axes[0], t.device)
            if ax is None:
                return t
            out = t.new_zeros(t.shape[:-1] + (ax[1],))
            out[..., ax[0]] = t
            return out
        r, c = self._axis(axes[0], t.device), self._axis(axes[1], t.device)
        R = r[1] if r else t.shape[-2]
        Cc = c[1] if c else t.shape[-1]
        out = t.new_zeros(t.shape[:-2] + (R, Cc))
        ri = r[0] if r else torch.arange(t.shape[-2], device=t.device)
        ci = c[0] if c else torch.arange(t.shape[-1], device=t.device)
        out[..., ri[:, None], ci[None, :]] = t
        return out

    def _unpad(self, g: Tensor, axes) -> Tensor:
        """the true-shaped part of a padded tensor (a gradient written by the library in its own shape)"""
        if len(axes) == 1:
            ax = self._axis(axes[0], g.device)
            return g if ax is None else g[..., ax[0]]
        r, c = self._axis(axes[0], g.device), self._axis(axes[1], g.device)
        ri = r[0] if r else torch.arange(g.shape[-2], device=g.device)
        ci = c[0] if c else torch.arange(g.shape[-1], device=g.device)
        return g[..., ri[:, None], ci[None, :]]

    def _packed_weights(self, device: torch.device) -> _Packed:
        """vs_weights* for the current parameter values; re-packed whenever any parameter was
        written (optimizer step, load_state_dict, .to()) — detected by (data_ptr, _version)."""
        if self._plan_error is not None:
            raise self._plan_error
        key = (device,) + tuple((t.data_ptr(), t._version) for t in self._tensors())
        if self._packed is not None and key == self._packed_key:
            return self._packed
        shape_key = (device, self.d_model, self.num_heads, self.num_layers, self.in_features,
                     self.pe_len if self.use_pos else 0, self.num_classes)
        lib = _lib.load()
        ts = []
        for t in self._tensors():
            if t.device != device:
                raise RuntimeError("SimNet parameters are on %s but the input is on %s" % (t.device, device))
            # (an fp32 contiguous tensor is used as it is: no detach / cast / contiguous objects per parameter and step)
            ts.append(t if (t.dtype == torch.float32 and t.is_contiguous()) else t.detach().to(torch.float32).contiguous())
        if self._plan:        # embedded model: the library sees zero-padded parameters of its own shape
            ts = [self._pad(t.detach(), ax).contiguous() for t, ax in zip(ts, self._tensor_axes())]
        reuse = self._packed is not None and self._packed_shape == shape_key
        P = _model_struct(_lib.ModelParams, ts, self.num_layers, self.use_pos)
        if self.use_pos:
            pe = self.embedding_layer.positional_encoding.pos_embedding
            pe_key = (pe.data_ptr(), pe._version)
            if reuse and pe_key == self._packed_pe_key:
                P.pos_embedding = None          # the table (a buffer) is unchanged: vs_weights_update keeps the packed copy
            self._packed_pe_key = pe_key
        desc = _lib.ModelDesc(self._lib_d, self.num_heads, self.num_layers, self.in_features,
                              self.pe_len if self.use_pos else 0, self.num_classes)
        with on_stream(device) as stream:
            if reuse:
                # parameters were written (optimizer step, load_state_dict): refill the existing device storage
                _lib.check(lib.vs_weights_update(self._packed.handle, C.byref(P), stream))
            else:
                out = C.c_void_p()
                _lib.check(lib.vs_weights_pack(C.byref(desc), C.byref(P), stream, C.byref(out)))
                self._packed, self._packed_shape = _Packed(out.value, device), shape_key
                if self._plan:
                    _lib.check(lib.vs_weights_set_norm_width(out.value, self.d_model))
        del ts      # stream-ordered: the async copies are already enqueued on the current stream
        self._packed_key = key
        return self._packed

    # ---- forward --------------------------------------------------------------------------
    def _needs_autograd(self, x: Tensor) -> bool:
        if not torch.is_grad_enabled():
            return False
        return self.training or x.requires_grad or any(p.requires_grad for p in self.parameters())

    def _forward_train(self, x: Tensor, mask: Optional[Tensor], lengths=None):
        """forward under autograd (``lengths``: of a packed batch): dropout (train mode only, like nn.Dropout) with a fresh seed
        drawn from torch's default CPU generator (so ``set_seed`` / ``torch.manual_seed``, reference utils.py:9-12, reproduces
        a run)."""
        p = self.drop_rate if self.training else 0.0
        p_embed = self.sparsity if (self.training and self.use_pos) else 0.0
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if (p > 0.0 or p_embed > 0.0) else 0
        params = [t for t in self._tensors() if isinstance(t, nn.Parameter)]
        x32 = x if x.dtype == torch.float32 else x.float()
        return _TrainForward.apply(self, x32, mask, lengths, p, p_embed, seed, self._train_flags(packed=lengths is not None), *params)

    def _check_table(self, longest: int) -> None:
        if self.use_pos and longest > self.pe_len:
            raise RuntimeError("T=%d exceeds the positional table (%d rows)" % (longest, self.pe_len))

    def _check_hip(self, x: Tensor) -> None:
        if not x.is_cuda:
            raise RuntimeError("SimNet runs on the MI355X HIP kernels only: move the module and its "
                               "input to a HIP device (there is no CPU path for the scorer)")

    def _check_padded(self, x: Tensor) -> None:
        """what ``forward`` and the attention maps refuse, in this order: the shape, a video longer than the table, a CPU tensor"""
        if x.dim() != 3 or x.size(2) != self.in_features:
            raise RuntimeError("expected x of shape [B, T, %d], got %s" % (self.in_features, tuple(x.shape)))
        self._check_table(x.size(1))
        self._check_hip(x)

    def forward(self, x: Tensor, mask=None, vis_attention=None, model_score: bool = False):
        """Same contract as reference ``SimNet.forward`` (simnet.py:32-45): returns
        ``(final_out [B,T,num_classes] raw logits, hidden [B,T,d])``; a non-Tensor ``mask`` is ignored
        (:38); ``vis_attention`` is ignored (:41); ``model_score`` selects ``intermediate`` which is the
        same tensor because ``module_score`` is empty."""
        self._check_padded(x)
        mask = mask if isinstance(mask, Tensor) else None
        if self.use_cls:
            return self._forward_cls(x, mask)
        if self._needs_autograd(x):
            return self._forward_train(x, mask)
        flags = (_lib.VS_FLAG_SIGMOID if self.fused_sigmoid else 0) | self._attention_flag()
        x32 = x if x.dtype == torch.float32 else x.float()
        packed = self._packed_weights(x.device)
        scores, hidden = torch.ops.vs_amd.score_frames(x32, mask, packed.handle, self._lib_d,
                                                       self.num_classes, flags, True)
        return scores, (hidden[..., :self.d_model] if self._plan else hidden)

    def _forward_cls(self, x: Tensor, mask: Optional[Tensor]):
        """``use_cls=True`` (simnet.py:47-51, 205-206, 214-216; no reference caller enables it): a learnable class token
        is prepended after the embedding, so the encoder sees T + 1 positions and both outputs have T + 1 rows.  Scoring
        only (no-grad).  One C call, ``vs_scorer_forward_cls``: the packed weights of the main path (cached, re-packed
        only when a parameter changes), the token row inserted by a kernel of the library - no per-call weight casts,
        no ``torch.cat``; every compute mode of the main path."""
        if self._needs_autograd(x):
            raise NotImplementedError("use_cls=True is supported for scoring (torch.no_grad / eval with frozen "
                                      "parameters) only; no reference caller trains with a class token")
        lib = _lib.load()
        B, T, _ = x.shape
        dev = x.device
        x32 = (x if x.dtype == torch.float32 else x.float()).contiguous()
        packed = self._packed_weights(dev)
        cls = self.embedding_layer.cls_token.detach()
        if cls.dtype != torch.float32 or not cls.is_contiguous():
            cls = cls.to(torch.float32).contiguous()
        m = mask_u8(mask)
        flags = (_lib.VS_FLAG_SIGMOID if self.fused_sigmoid else 0) | self._attention_flag()
        scores = torch.empty((B, T + 1, self.num_classes), dtype=torch.float32, device=dev)
        hidden = torch.empty((B, T + 1, self._lib_d), dtype=torch.float32, device=dev)
        if self._plan:
            cls = self._pad(cls, ("res",)).contiguous()
        with on_stream(dev) as st:
            ws = scratch(lib.vs_scorer_workspace_bytes_cls(packed.handle, B, T), dev, floor=256)
            _lib.check(lib.vs_scorer_forward_cls(packed.handle, x32.data_ptr(), ptr(m), cls.data_ptr(), B, T, flags,
                                                 scores.data_ptr(), hidden.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return scores, (hidden[..., :self.d_model] if self._plan else hidden)

    @torch.no_grad()
    def score(self, x: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        """Sigmoid importance scores [B,T] in one launch sequence: the ``val_step`` head
        (train.py:143-144) with the sigmoid fused and the hidden-state store skipped."""
        if self.num_classes != 1:
            raise RuntimeError("score() needs num_classes == 1")
        if self.use_cls:                                    # T + 1 scores (class token first), sigmoid fused as well
            prev, self.fused_sigmoid = self.fused_sigmoid, True
            try:
                s, _ = self._forward_cls(x, mask if isinstance(mask, Tensor) else None)
            finally:
                self.fused_sigmoid = prev
            return s.squeeze(-1)
        x32 = x if x.dtype == torch.float32 else x.float()
        packed = self._packed_weights(x.device)
        scores, _ = torch.ops.vs_amd.score_frames(x32, mask, packed.handle, self._lib_d, 1,
                                                  _lib.VS_FLAG_SIGMOID | self._attention_flag(), False)
        return scores.squeeze(-1)

    # ---- attention maps on request (include/vs_inspect.h) ----------------------------------
    def _select_layers(self, layers):
        """(the selected layers in the caller's order, the same ascending - the order the C entries take)"""
        L = self.num_layers
        want = list(range(L)) if layers is None else [int(l) for l in layers]
        sel = [l + L if l < 0 else l for l in want]
        if not sel or any(l < 0 or l >= L for l in sel) or len(set(sel)) != len(sel):
            raise IndexError("layers must be distinct indices of the %d encoder layers, got %r" % (L, want))
        return sel, sorted(sel)

    def _inspect(self, x: Tensor, mask, layers, want_maps: bool):
        """One ``vs_inspect_forward`` call: the exact fp32 eval forward plus the attention-map kernels on the q / k planes of
        the selected layers.  Returns (logits, maps or None, received or None, entropy or None), stacked over the layers."""
        self._check_padded(x)
        mask = mask if isinstance(mask, Tensor) else None
        sel, asc = self._select_layers(layers)
        lib = _lib.load()
        B, T, _ = x.shape
        dev = x.device
        N, H = T + (1 if self.use_cls else 0), self.num_heads
        x32 = (x if x.dtype == torch.float32 else x.float()).contiguous()
        packed = self._packed_weights(dev)
        cls = None
        if self.use_cls:
            cls = self.embedding_layer.cls_token.detach().to(torch.float32).contiguous()
            if self._plan:
                cls = self._pad(cls, ("res",)).contiguous()
        m = mask_u8(mask)
        scores = torch.empty((B, N, self.num_classes), dtype=torch.float32, device=dev)
        maps = torch.empty((len(asc), B, H, N, N), dtype=torch.float32, device=dev) if want_maps else None
        received = None if want_maps else torch.empty((len(asc), B, H, N), dtype=torch.float32, device=dev)
        entropy = None if want_maps else torch.empty((len(asc), B, H, N), dtype=torch.float32, device=dev)
        host_layers = (C.c_int32 * len(asc))(*asc)
        with on_stream(dev) as st:
            ws = scratch(lib.vs_inspect_workspace_bytes(packed.handle, B, T, 1 if self.use_cls else 0), dev, floor=256)
            _lib.check(lib.vs_inspect_forward(packed.handle, x32.data_ptr(), ptr(m), ptr(cls), B, T, host_layers, len(asc),
                                              scores.data_ptr(), None, ptr(maps), ptr(received), ptr(entropy),
                                              ws.data_ptr(), ws.numel(), st))
        if sel != asc:      # the caller's order
            order = torch.tensor([asc.index(l) for l in sel], device=dev)
            maps, received, entropy = (t if t is None else t.index_select(0, order) for t in (maps, received, entropy))
        return scores, maps, received, entropy

    @torch.no_grad()
    def attention_maps(self, x: Tensor, mask=None, layers=None):
        """The softmax weights of the self-attention layers (reference simnet.py:155-164, the ``attention_maps`` list of
        :112-113): returns ``(logits, maps)``, ``maps`` a list with one ``[B, H, N, N]`` fp32 device tensor per selected
        layer (``N = T``, or ``T + 1`` with ``use_cls``, token first).  ``layers=None`` selects every layer; negative
        indices count from the last.  ``maps[l][b, h, i, j]`` is the weight query ``i`` gives key ``j``: taken before
        dropout (the reference's tensor in eval mode), a masked key column is exactly 0, padded query rows are computed
        like any other row.  ``B * H * N * N * 4`` bytes per layer: use ``attention_summary`` for long videos.

        The maps describe the EXACT fp32 path: whatever ``set_compute_dtype`` / ``set_latency_mode`` / ``fused_sigmoid``
        / ``model.training`` say, this call runs the default exact kernels in eval semantics (it changes none of those
        settings), and ``logits`` are the raw logits of ``forward`` in the default mode, bit for bit.  Unlike the
        reference the tensors stay on the device.  No autograd, no CPU path; ragged batches: ``attention_maps_packed``."""
        scores, maps, _, _ = self._inspect(x, mask, layers, True)
        return scores, list(maps.unbind(0))

    @torch.no_grad()
    def attention_summary(self, x: Tensor, mask=None, layers=None):
        """Two reductions of the attention maps that never store ``[N, N]`` (any video length): returns
        ``(logits, received, entropy)``, both ``[n_layers, B, H, N]`` fp32 device tensors.  ``received[l, b, h, j]`` is the
        mean weight frame ``j`` receives from the video's non-padding frames (sums to 1 over ``j``; 0 for a masked frame);
        ``entropy[l, b, h, i]`` is the entropy of frame ``i``'s weights in nats (0: it attends to one frame; ``log n``:
        uniform over the ``n`` valid frames).  Same arithmetic, modes and limits as ``attention_maps``."""
        scores, _, received, entropy = self._inspect(x, mask, layers, False)
        return scores, received, entropy

    def _inspect_packed(self, x: Tensor, lengths, layers, want_maps: bool):
        """One ``vs_inspect_forward_packed`` call.  Returns (logits [M, C], lengths, maps [n_layers, H * sum T^2] or None,
        received [n_layers, H, M] or None, entropy or None), the layers in the caller's order.  Refuses, in this order and all
        before any launch: a class token, head dim 256, the shape, a video longer than the table, the layers, a CPU tensor."""
        if self.use_cls:
            raise NotImplementedError("packed batches are not available with use_cls=True")
        if self._lib_dh not in (32, 64, 128):
            raise RuntimeError("packed batches need head_dim 32, 64 or 128 (got %d)" % self._lib_dh)
        lengths, host = host_lengths(lengths)
        if x.dim() != 2 or x.size(1) != self.in_features or x.size(0) != sum(lengths):
            raise RuntimeError("expected x of shape [sum(lengths)=%d, %d], got %s" % (sum(lengths), self.in_features, tuple(x.shape)))
        if not lengths or min(lengths) <= 0:
            raise RuntimeError("lengths must be positive, got %r" % (lengths,))
        self._check_table(max(lengths))
        sel, asc = self._select_layers(layers)
        self._check_hip(x)
        lib = _lib.load()
        dev, M, B, H = x.device, x.size(0), len(lengths), self.num_heads
        x32 = (x if x.dtype == torch.float32 else x.float()).contiguous()
        packed = self._packed_weights(dev)
        scores = torch.empty((M, self.num_classes), dtype=torch.float32, device=dev)
        maps = torch.empty((len(asc), H * sum(t * t for t in lengths)), dtype=torch.float32, device=dev) if want_maps else None
        received = None if want_maps else torch.empty((len(asc), H, M), dtype=torch.float32, device=dev)
        entropy = None if want_maps else torch.empty((len(asc), H, M), dtype=torch.float32, device=dev)
        host_layers = (C.c_int32 * len(asc))(*asc)
        with on_stream(dev) as st:
            dev_len = torch.tensor(lengths, dtype=torch.int32, device=dev)
            ws = scratch(lib.vs_inspect_workspace_bytes_packed(packed.handle, host, B), dev, floor=256)
            _lib.check(lib.vs_inspect_forward_packed(packed.handle, x32.data_ptr(), host, dev_len.data_ptr(), B, host_layers, len(asc),
                                                     scores.data_ptr(), None, ptr(maps), ptr(received), ptr(entropy),
                                                     ws.data_ptr(), ws.numel(), st))
        if sel != asc:      # the caller's order
            order = torch.tensor([asc.index(l) for l in sel], device=dev)
            maps, received, entropy = (t if t is None else t.index_select(0, order) for t in (maps, received, entropy))
        return scores, lengths, maps, received, entropy

    @torch.no_grad()
    def attention_maps_packed(self, x: Tensor, lengths, layers=None):
        """``attention_maps`` on a RAGGED batch without padding: x [sum(lengths), in_features] = the videos' frames concatenated
        (``forward_packed``).  Returns ``(logits [M, num_classes], maps)``: ``maps[l][b]`` is the ``[H, T_b, T_b]`` fp32 weights
        of video ``b`` in the ``l``-th selected layer, a view into ONE allocation per call of ``n_layers * H * sum(T_b^2)``
        floats - where the padded call allocates ``n_layers * B * H * Tmax^2``.  No padded row or masked column exists.  Same
        semantics as ``attention_maps``: exact fp32 eval arithmetic whatever the modes say (none is changed), ``logits`` are the
        bits of ``forward_packed`` in the default mode, ``layers`` as there.  A video's maps are bit-identical whatever it is
        packed with.  Head dim 32 / 64 / 128, no class token (as ``forward_packed``)."""
        scores, lengths, maps, _, _ = self._inspect_packed(x, lengths, layers, True)
        H, out = self.num_heads, []
        for layer in maps.unbind(0):
            views, off = [], 0
            for t in lengths:
                views.append(layer[off:off + H * t * t].view(H, t, t))
                off += H * t * t
            out.append(views)
        return scores, out

    @torch.no_grad()
    def attention_summary_packed(self, x: Tensor, lengths, layers=None):
        """``attention_summary`` on a packed ragged batch (see ``attention_maps_packed``): returns ``(logits [M, num_classes],
        received [n_layers, H, M], entropy [n_layers, H, M])``, packed like the frames: video ``b`` = columns
        ``sum(lengths[:b]) ...``.  ``received`` sums to 1 over each video's own frames.  Never stores ``[T, T]``."""
        scores, _, _, received, entropy = self._inspect_packed(x, lengths, layers, False)
        return scores, received, entropy

    def _check_head_dim(self, arithmetic: str) -> None:
        ok = _ATTENTION_HEAD_DIMS[arithmetic]
        if self._lib_dh not in ok:
            raise ValueError("%s attention needs head_dim in %s, got %d" % (arithmetic, ok, self._lib_dh))

    @property
    def attention_dtype(self) -> str:
        return self._attention_dtype

    @attention_dtype.setter
    def attention_dtype(self, value: str) -> None:
        if value not in ("fp32", "bf16", "fp16x3"):
            raise ValueError("attention_dtype must be 'fp32', 'bf16' or 'fp16x3', got %r" % (value,))
        if value != "fp32":
            self._check_head_dim(value)
        self._attention_dtype = value

    @property
    def linear_dtype(self) -> str:
        return self._linear_dtype

    @linear_dtype.setter
    def linear_dtype(self, value: str) -> None:
        if value not in ("fp32", "bf16", "fp16x3"):
            raise ValueError("linear_dtype must be 'fp32', 'bf16' or 'fp16x3', got %r" % (value,))
        self._linear_dtype = value

    def set_compute_dtype(self, value: str) -> "SimNet":
        """'fp32' (default: exact fp32 MFMA), 'fp16x3' (fp32 EMULATED on the f16 matrix pipe: operands split into
        hi + lo halves, three products, fp32 accumulate - same 1e-4 parity, ~2x faster; operands < 65504) or 'bf16'
        (BASELINE config 5: operands rounded to bf16, logits move by ~4e-3).  Tensors, softmax, LayerNorm and the
        score head stay fp32 in every mode."""
        # models with head dim 128 (M-B) take what exists for them: fp16x3 -> every Linear emulated, attention exact;
        # bf16 -> every product on the bf16 pipe (head dim 128 has a bf16 attention; d_model > 256 runs the plain bf16
        # GEMMs + the row LayerNorm pass instead of the fused layer kernels)
        head_ok = self._lib_dh in _ATTENTION_HEAD_DIMS["fp16x3"]
        if value not in ("fp32", "fp16x3", "bf16"):
            raise ValueError("compute dtype must be 'fp32', 'fp16x3' or 'bf16', got %r" % (value,))
        if value == "bf16":
            self.attention_dtype = "bf16" if self._lib_dh <= 128 else "fp32"      # (head dim 256: exact attention only)
        else:
            self.attention_dtype = value if (head_ok or value == "fp32") else "fp32"
        self.linear_dtype = value
        return self

    def _note_train_arithmetic(self, tflags: int, fmt: int, frames: int) -> None:
        """Records which arithmetic the last training forward actually ran (``last_train_dtype``) and says so - once - when a
        low-precision request was not honoured (the library keeps batches below VS_TRAIN_LP_MIN_ROWS frames on the exact kernels)."""
        form = _lib.train_form(fmt)
        self.last_train_dtype = form.dtype(form.lp or form.lpa)
        if tflags and not (form.lp or form.lpa) and not getattr(self, "_warned_train_dtype", False):
            import warnings
            self._warned_train_dtype = True
            warnings.warn("set_train_dtype(%r) was requested but this batch (%d frames) ran on the exact fp32 kernels: the "
                          "low-precision training kernels apply above VS_TRAIN_LP_MIN_ROWS frames per batch (see "
                          "SimNet.last_train_dtype after any training forward)" % (self._train_dtype, frames), RuntimeWarning)

    def set_train_dtype(self, value: str, packed_attention: bool = False) -> "SimNet":
        """Arithmetic of the TRAINING path's matrix products (forward Linears, dgrad and wgrad GEMMs): 'fp32' (default:
        exact fp32 MFMA, gradients at 1e-6 of the float64 truth) or 'bf16' - the counterpart of the reference's
        ``with amp.autocast():`` (train.py:120, pretrain.py:59): operands rounded to bf16, fp32 accumulation, and - as
        under autocast - LayerNorm, softmax statistics and the loss in fp32.  The attention products (forward and both
        backward kernels) run on the bf16 pipe too (head dim 32 / 64 / 128), and the tensors that are only ever bf16 matrix
        operands (q / k / v, the MLP hidden tensor and its gradient, the attention gradients) are stored as bf16.  Applies
        above VS_TRAIN_LP_MIN_ROWS frames per batch (default 1024; ``last_train_dtype`` says what a forward really ran).
        Gradients within ~2e-2 relative L2 of the float64 truth (tests/tolerances.py TRAIN_LP_*).
        'fp16': the same structure with IEEE fp16 as the 16-bit type - the reference's own autocast type on CUDA - 11
        significant bits, gradients ~8x closer to the truth (TRAIN_FP16_*), but a range of 65 504 / 6e-8: train with a loss
        scale exactly as the reference does (``torch.amp.GradScaler``, train.py:60,126-128) - ``scaler.scale(loss).backward()``
        reaches these kernels as a scaled ``d_scores``, an overflow surfaces as inf / NaN gradients and GradScaler skips
        the step and halves the scale.
        Packed ragged batches (``forward_packed_train``): the Linears, dgrad and wgrad follow this setting; the packed attention
        is exact fp32 in every mode unless ``packed_attention=True`` is given with 'bf16' / 'fp16': then its products run on that
        16-bit pipe as well (head dim 32 / 64 / 128, above VS_TRAIN_LP_MIN_ROWS packed frames; q / k / v and the attention
        gradients stay fp32-stored; ``last_packed_attention_dtype`` says what a packed forward really ran).  Opt-in: the
        default leaves every packed step bit-identical to what it was.  With 'fp32' the keyword has no effect."""
        if value not in ("fp32", "bf16", "fp16"):
            raise ValueError("train dtype must be 'fp32', 'bf16' or 'fp16', got %r" % (value,))
        packed_attention = bool(packed_attention) and value != "fp32"
        if packed_attention:
            self._check_head_dim(value)
        self._train_dtype = value
        self._packed_attention = packed_attention
        return self

    @property
    def last_packed_attention_dtype(self) -> str:
        """Arithmetic of the attention products of the last ``forward_packed_train`` ('fp32' / 'bf16' / 'fp16'), from the format
        word the library published for it; 'fp32' before any."""
        return self._last_packed_attention_dtype

    def _train_flags(self, packed: bool = False) -> int:
        tflags = (_lib.VS_TRAIN_FLAG_BF16_LINEAR | _lib.VS_TRAIN_FLAG_BF16_ATTENTION) if self._train_dtype in ("bf16", "fp16") else 0
        if packed and tflags and self._packed_attention:
            tflags |= _lib.VS_TRAIN_FLAG_PACKED_LP_ATTENTION
        return tflags | (_lib.VS_TRAIN_FLAG_FP16 if self._train_dtype == "fp16" else 0)

    def forward_packed_train(self, x: Tensor, lengths):
        """``forward`` under autograd on a RAGGED batch without padding: x [sum(lengths), in_features] = the videos' frames
        concatenated (``data.collate_fn_train_packed``).  Returns (logits [Mtot, num_classes], hidden [Mtot, d_model]), both
        differentiable; video i = rows sum(lengths[:i]) ...  Where the reference pads every batch to its longest video with
        the 1000.0 sentinel and masks (dataset.py:157-161, train.py:118), no padded row is computed here - forward or
        backward - and the activation record scales with sum(lengths): masked keys and masked loss rows contribute exactly
        zero to every gradient, so with ``losses.mse_packed_loss`` the step equals the padded one.  With dropout off a
        video's outputs are bit-identical to running it alone.  Dropout is active iff ``self.training`` (seed drawn like
        ``forward``'s).  ``set_train_dtype("bf16" | "fp16")`` runs the Linears, dgrad and wgrad in low precision above
        VS_TRAIN_LP_MIN_ROWS packed frames; the packed ATTENTION stays exact fp32 unless ``set_train_dtype(...,
        packed_attention=True)`` opted in (head dim 32 / 64 / 128; ``last_train_dtype`` names the arithmetic of the Linears,
        ``last_packed_attention_dtype`` that of the attention).  Every head dim of the padded training path; embedded shapes
        work; no class token."""
        if self.use_cls:
            raise NotImplementedError("packed batches are not available with use_cls=True")
        self._check_hip(x)
        lengths = [int(t) for t in lengths]
        if x.dim() != 2 or x.size(1) != self.in_features or x.size(0) != sum(lengths):
            raise RuntimeError("expected x of shape [sum(lengths)=%d, %d], got %s" % (sum(lengths), self.in_features, tuple(x.shape)))
        if not lengths or min(lengths) <= 0:
            raise RuntimeError("lengths must be positive, got %r" % (lengths,))
        self._check_table(max(lengths))
        return self._forward_train(x, None, lengths)

    @torch.no_grad()
    def forward_packed(self, x: Tensor, lengths, want_hidden: bool = True):
        """Scores a RAGGED batch without padding: x [sum(lengths), in_features] = the videos' frames concatenated.
        Returns (logits [Mtot, num_classes], hidden [Mtot, d_model]); video i = rows sum(lengths[:i]) ...  The reference
        pads with the 1000.0 sentinel and masks (dataset.py:157-161); here no padded row is computed, and each video's
        result is bit-identical to scoring it alone (fp32 and fp16x3 modes).  Head dim 32 / 64 / 128."""
        if not x.is_cuda:
            raise RuntimeError("SimNet scoring runs on the MI355X HIP kernels only (no CPU path for the scorer)")
        if self.use_cls:
            raise NotImplementedError("packed batches are not available with use_cls=True")
        if self.use_pos:
            self._check_table(max(int(t) for t in lengths))
        packed = self._packed_weights(x.device)
        x32 = x if x.dtype == torch.float32 else x.float()
        flags = (_lib.VS_FLAG_SIGMOID if self.fused_sigmoid else 0) | self._attention_flag()
        scores, hidden = score_frames_packed(x32, lengths, packed.handle, self._lib_d, self.num_classes, flags, want_hidden)
        return scores, (hidden[..., :self.d_model] if (self._plan and want_hidden) else hidden)

    @torch.no_grad()
    def score_packed(self, x: Tensor, lengths) -> Tensor:
        """Sigmoid importance scores [Mtot] of a packed ragged batch (see forward_packed)."""
        if self.num_classes != 1:
            raise RuntimeError("score_packed() needs num_classes == 1")
        if self.use_cls:
            raise NotImplementedError("packed batches are not available with use_cls=True")
        packed = self._packed_weights(x.device)
        x32 = x if x.dtype == torch.float32 else x.float()
        s, _ = score_frames_packed(x32, lengths, packed.handle, self._lib_d, 1,
                                   _lib.VS_FLAG_SIGMOID | self._attention_flag(), False)
        return s.squeeze(-1)

    def set_latency_mode(self, on: bool = True) -> "SimNet":
        """Opt-in latency mode for reference-sized scoring calls (one T = 320 video per forward, ``train.py:139-148``,
        ``generate_summary_image.py:62-67``): the exact-fp32 K >= 512 Linears and the out-projection are split over K across
        more CUs and LayerNorm runs as a row pass (``VS_FLAG_SPLITK``).  Deterministic, batch-independent and within ~1e-6 of
        the default kernels (goldens at 1e-4) - but a different summation tree: a video scored alone in this mode is no longer
        bit-identical to the same video scored inside a large batch, which the default guarantees.  No effect above
        VS_SKINNY_ROWS rows, in the low-precision modes, or for packed / class-token calls."""
        self.latency_mode = bool(on)
        return self

    def _attention_flag(self) -> int:
        return ((_lib.VS_FLAG_SPLITK if self.latency_mode else 0)
                | (_lib.VS_FLAG_BF16_ATTENTION if self._attention_dtype == "bf16" else 0)
                | (_lib.VS_FLAG_F16X3_ATTENTION if self._attention_dtype == "fp16x3" else 0)
                | (_lib.VS_FLAG_BF16_LINEAR if self._linear_dtype == "bf16" else 0)
                | (_lib.VS_FLAG_F16X3_LINEAR if self._linear_dtype == "fp16x3" else 0))
