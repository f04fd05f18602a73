"""``mse_with_mask_loss`` — drop-in for the reference training loss, on the HIP kernels.

Same signature and value as reference ``src/utils/utils.py:45-56`` (called at ``train.py:122``):
``((output.squeeze(2) - targets) * scale) ** 2`` with ``scale = 0`` on masked frames, averaged (``reduction="avg"``)
or summed over ALL ``B*T`` entries.  Forward (two-stage fixed-order reduction) and backward are kernels of
``libvsscore.so`` (``include/vs_train.h``: ``vs_mse_mask_loss_forward`` / ``_backward``); HIP tensors only.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib
from ._call import mask_u8, on_stream, ptr


class _MseMask(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, output: Tensor, targets: Tensor, mask, mean: bool):
        lib = _lib.load()
        o, t = output.contiguous(), targets.contiguous().float()
        if o.numel() != t.numel():
            raise RuntimeError("output %s and targets %s differ in size" % (tuple(output.shape), tuple(targets.shape)))
        m = mask_u8(mask)
        if m is not None and m.numel() != o.numel():
            raise RuntimeError("mask %s does not match output %s" % (tuple(mask.shape), tuple(output.shape)))
        loss = torch.empty((), dtype=torch.float32, device=o.device)
        with on_stream(o.device) as stream:
            scratch = torch.empty((256,), dtype=torch.float32, device=o.device)
            _lib.check(lib.vs_mse_mask_loss_forward(o.data_ptr(), t.data_ptr(), ptr(m),
                                                    o.numel(), int(mean), scratch.data_ptr(), loss.data_ptr(), stream))
        ctx.save_for_backward(o, t, m)
        ctx.mean, ctx.shape = bool(mean), output.shape
        return loss

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_loss):
        lib = _lib.load()
        o, t, m = ctx.saved_tensors
        d_out = torch.empty_like(o)
        g = d_loss.contiguous().float()
        with on_stream(o.device) as stream:
            _lib.check(lib.vs_mse_mask_loss_backward(o.data_ptr(), t.data_ptr(), ptr(m),
                                                     g.data_ptr(), o.numel(), int(ctx.mean), d_out.data_ptr(), stream))
        return d_out.view(ctx.shape), None, None, None


def mse_with_mask_loss(output: Tensor, targets: Tensor, mask, reduction: str = "avg") -> Tensor:
    """output [B,T,1] (the scorer's logits), targets [B,T], mask bool [B,T] (True = padded frame) -> scalar loss."""
    if not output.is_cuda:
        raise RuntimeError("mse_with_mask_loss runs on the MI355X HIP kernels only (HIP tensors)")
    mk = mask if isinstance(mask, Tensor) else None
    return _MseMask.apply(output, targets, mk, reduction == "avg")


class _MsePacked(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, output: Tensor, targets: Tensor, denom: float):
        lib = _lib.load()
        o, t = output.contiguous(), targets.contiguous().float()
        if o.numel() != t.numel():
            raise RuntimeError("output %s and targets %s differ in size" % (tuple(output.shape), tuple(targets.shape)))
        loss = torch.empty((), dtype=torch.float32, device=o.device)
        with on_stream(o.device) as stream:
            scratch = torch.empty((256,), dtype=torch.float32, device=o.device)
            _lib.check(lib.vs_mse_packed_loss_forward(o.data_ptr(), t.data_ptr(), o.numel(), float(denom), scratch.data_ptr(),
                                                      loss.data_ptr(), stream))
        ctx.save_for_backward(o, t)
        ctx.denom, ctx.shape = float(denom), output.shape
        return loss

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_loss):
        lib = _lib.load()
        o, t = ctx.saved_tensors
        d_out = torch.empty_like(o)
        g = d_loss.contiguous().float()
        with on_stream(o.device) as stream:
            _lib.check(lib.vs_mse_packed_loss_backward(o.data_ptr(), t.data_ptr(), g.data_ptr(), o.numel(), ctx.denom,
                                                       d_out.data_ptr(), stream))
        return d_out.view(ctx.shape), None, None


def mse_packed_loss(output: Tensor, targets: Tensor, lengths, reduction: str = "avg") -> Tensor:
    """The training loss of a PACKED ragged batch: output [Mtot, 1] (or [Mtot]) from ``SimNet.forward_packed_train``, targets
    [Mtot], lengths the videos' frame counts.  Value and gradient equal the reference's ``mse_with_mask_loss`` (utils.py:45-56)
    on the padded batch of the same videos: ``"avg"`` divides the sum of squares by ``B * max(lengths)``, because the
    reference averages over ALL ``B*T`` entries, the masked (zero) ones included; anything else sums."""
    if not output.is_cuda:
        raise RuntimeError("mse_packed_loss runs on the MI355X HIP kernels only (HIP tensors)")
    lengths = [int(t) for t in lengths]
    if output.numel() != sum(lengths):
        raise RuntimeError("output %s does not hold sum(lengths)=%d entries" % (tuple(output.shape), sum(lengths)))
    denom = float(len(lengths) * max(lengths)) if reduction == "avg" else 1.0
    return _MsePacked.apply(output, targets, denom)
