"""Counterpart of the reference's ``model.PretrainModel`` (src/model/simnet_pretrain.py:12-100), the consumer of
the scorer's hidden output in ``pretrain.py``: same constructor, same parameter names
(``encoder.*`` = SimNet, ``video_transform.{weight,bias}``), same ``forward`` signature and return triple
``(distillation loss, centering loss, repelling loss)``.

``forward`` runs on the HIP kernels end to end: the encoder is the HIP training path (``simnet._TrainForward``) and
everything below it - ``video_transform``, the repelling loss, the masked score-softmax pooling, the centering penalty
and the soft cross-entropy, forward and backward - is ``_PretrainHead``, a ``torch.autograd.Function`` over
``vs_pretrain_head_forward / _backward`` (``include/vs_train.h``, kernels ``csrc/vs_pretrain_kernels.hip``).  There is
no PyTorch fallback: CPU tensors raise.  ``forward_packed`` is the same step on a packed ragged batch (no sentinel rows, no
mask): ``SimNet.forward_packed_train`` under ``_PretrainHeadPacked``.

One algorithmic change.  The reference materialises the [B,T,T] cosine-similarity tensor to average its off-diagonal
(simnet_pretrain.py:56-69); the same number is

    sum_{i != j} x^_i . x^_j = || sum_i x^_i ||^2 - sum_i || x^_i ||^2        (x^ = masked, normalised rows)

which costs O(T d) instead of O(T^2 d) time and memory (T = 2000, d = 512: 16 MB of [T,T] per video avoided in
the forward and again in the backward), and differs from the reference only by fp32 rounding.  The methods
``cross_entropy_loss`` / ``entropy`` / ``repelling_loss`` are kept with the reference's signatures for callers that use
them on their own tensors; ``forward`` does not go through them.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import _lib
from ._call import host_lengths, mask_u8, on_stream, ptr, scratch
from .simnet import SimNet


class _PretrainHead(torch.autograd.Function):
    """(hidden [B,T,d], logits [B,T,1], vid [B,F], mask, video_transform.weight, .bias) -> losses [3]."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)        # pretrain.py:59 calls under autocast
    def forward(ctx, hidden, logits, vid, mask, weight, bias, temp, entropy):
        lib = _lib.load()
        B, T, d = hidden.shape
        Fo = weight.shape[0]
        hidden, logits, vid = hidden.contiguous(), logits.contiguous(), vid.contiguous()
        w, bvec = weight.detach().contiguous(), bias.detach().contiguous()
        m = mask_u8(mask)
        dev = hidden.device
        feats = torch.empty((B, T, Fo), dtype=torch.float32, device=dev)
        losses = torch.empty((3,), dtype=torch.float32, device=dev)
        with on_stream(dev) as stream:
            state = scratch(lib.vs_pretrain_head_state_bytes(B, T, Fo), dev)
            _lib.check(lib.vs_pretrain_head_forward(hidden.data_ptr(), logits.data_ptr(), ptr(m),
                                                    vid.data_ptr(), w.data_ptr(), bvec.data_ptr(), B, T, d, Fo, float(temp),
                                                    int(entropy), feats.data_ptr(), state.data_ptr(), losses.data_ptr(), stream))
        ctx.save_for_backward(hidden, logits, vid, m, w, feats, state)
        ctx.cfg = (float(temp), int(entropy), logits.shape)
        return losses

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_losses):
        lib = _lib.load()
        hidden, logits, vid, m, w, feats, state = ctx.saved_tensors
        temp, entropy, lshape = ctx.cfg
        B, T, d = hidden.shape
        Fo = w.shape[0]
        dev = hidden.device
        g = d_losses.contiguous().float()
        d_hidden, d_logits = torch.empty_like(hidden), torch.empty((B, T), dtype=torch.float32, device=dev)
        d_w, d_b = torch.empty_like(w), torch.empty((Fo,), dtype=torch.float32, device=dev)
        with on_stream(dev) as stream:
            ws = scratch(lib.vs_pretrain_head_workspace_bytes(B, T, d, Fo), dev)
            _lib.check(lib.vs_pretrain_head_backward(hidden.data_ptr(), logits.data_ptr(), ptr(m),
                                                     vid.data_ptr(), w.data_ptr(), feats.data_ptr(), state.data_ptr(),
                                                     g.data_ptr(), B, T, d, Fo, temp, entropy, d_hidden.data_ptr(),
                                                     d_logits.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), stream))
        return d_hidden, d_logits.view(lshape), None, None, d_w, d_b, None, None


def _device_lengths(lengths, device) -> Tensor:
    """``lengths`` as int32 on ``device``, copied from page-locked memory without blocking the host.  (A copy from pageable
    memory is ordered after everything already enqueued on the stream and holds the host until it is done: in the middle of
    a step - below the encoder's forward - that would drain the queue the host has built up.)"""
    return torch.tensor(lengths, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


class _PretrainHeadPacked(torch.autograd.Function):
    """(hidden [Mtot,d], logits [Mtot,1], vid [B,F], lengths, ref_len, video_transform.weight, .bias) -> losses [3]: the head on
    a packed ragged batch (``vs_pretrain_head_forward_packed / _backward_packed``), no padded row in any pass.  Exact fp32.
    ``lengths_dev``: the lengths as an int32 device tensor when the caller has one already (None: copied here)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, hidden, logits, vid, lengths, ref_len, weight, bias, temp, entropy, lengths_dev=None):
        lib = _lib.load()
        lengths, host = host_lengths(lengths)
        Bv, (M, d) = len(lengths), hidden.shape
        Fo = weight.shape[0]
        if M != sum(lengths) or logits.numel() != M or tuple(vid.shape) != (Bv, Fo):
            raise RuntimeError("packed pretrain head: hidden %s / logits %s / vid %s do not match lengths (sum %d, B %d, F %d)"
                               % (tuple(hidden.shape), tuple(logits.shape), tuple(vid.shape), sum(lengths), Bv, Fo))
        hidden, logits, vid = hidden.contiguous(), logits.contiguous(), vid.contiguous()
        w, bvec = weight.detach().contiguous(), bias.detach().contiguous()
        dev = hidden.device
        feats = torch.empty((M, Fo), dtype=torch.float32, device=dev)
        losses = torch.empty((3,), dtype=torch.float32, device=dev)
        with on_stream(dev) as stream:
            dev_len = _device_lengths(lengths, dev) if lengths_dev is None else lengths_dev
            # (invalid lengths / F give 0 bytes: the forward call below says why)
            state = scratch(lib.vs_pretrain_head_state_bytes_packed(host, Bv, Fo), dev, floor=256)
            _lib.check(lib.vs_pretrain_head_forward_packed(hidden.data_ptr(), logits.data_ptr(), host, dev_len.data_ptr(), Bv,
                                                           int(ref_len), vid.data_ptr(), w.data_ptr(), bvec.data_ptr(), d, Fo,
                                                           float(temp), int(entropy), feats.data_ptr(), state.data_ptr(),
                                                           losses.data_ptr(), stream))
        ctx.save_for_backward(hidden, logits, vid, dev_len, w, feats, state)
        ctx.cfg = (float(temp), int(entropy), logits.shape, tuple(lengths), int(ref_len))
        return losses

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, d_losses):
        lib = _lib.load()
        hidden, logits, vid, dev_len, w, feats, state = ctx.saved_tensors
        temp, entropy, lshape, lengths, ref_len = ctx.cfg
        Bv, (M, d) = len(lengths), hidden.shape
        Fo = w.shape[0]
        dev = hidden.device
        _, host = host_lengths(lengths)
        g = d_losses.contiguous().float()
        d_hidden, d_logits = torch.empty_like(hidden), torch.empty((M,), dtype=torch.float32, device=dev)
        d_w, d_b = torch.empty_like(w), torch.empty((Fo,), dtype=torch.float32, device=dev)
        with on_stream(dev) as stream:
            ws = scratch(lib.vs_pretrain_head_workspace_bytes_packed(host, Bv, d, Fo), dev)
            _lib.check(lib.vs_pretrain_head_backward_packed(hidden.data_ptr(), logits.data_ptr(), host, dev_len.data_ptr(), Bv,
                                                            ref_len, vid.data_ptr(), w.data_ptr(), feats.data_ptr(),
                                                            state.data_ptr(), g.data_ptr(), d, Fo, temp, entropy,
                                                            d_hidden.data_ptr(), d_logits.data_ptr(), d_w.data_ptr(),
                                                            d_b.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return d_hidden, d_logits.view(lshape), None, None, None, d_w, d_b, None, None, None


class PretrainModel(nn.Module):
    def __init__(self, feature_dim: int = 256, sparsity: float = 0.0, sharpening_t=0.4, **kwargs):
        super().__init__()
        self.feature_dim = feature_dim                      # simnet_pretrain.py:24-26
        self.sparsity = sparsity
        self.sharpening_t = sharpening_t
        # the encoder never gets `sparsity` (hard-wired 0., simnet_pretrain.py:30)
        self.encoder = SimNet(sparsity=0., use_cls=False, d_model=feature_dim, **kwargs)
        self.video_transform = nn.Linear(feature_dim, 512)  # simnet_pretrain.py:33

    def cross_entropy_loss(self, x1: Tensor, x2: Tensor) -> Tensor:
        """simnet_pretrain.py:35-41: mean over ALL elements of -softmax(x2) * log softmax(x1)."""
        return (-F.softmax(x2, dim=1) * F.log_softmax(x1, dim=1)).mean()

    def entropy(self, x: Tensor, mask=None) -> Tensor:
        """simnet_pretrain.py:43-47 (x log x, masked positions zeroed, mean over frames then over the rest)."""
        x = x * torch.log(x)
        if isinstance(mask, Tensor):
            x = x.masked_fill(mask, 0.)
        return x.mean(dim=1).mean()

    def repelling_loss(self, x: Tensor, mask) -> Tensor:
        """simnet_pretrain.py:49-71: average cosine similarity between different frames (masked frames count as
        zero rows but stay in the T^2 denominator), without the [T,T] tensor - see the module docstring."""
        n_frames = x.size(1)
        if isinstance(mask, Tensor):
            x = x * (mask == False).unsqueeze(2)            # noqa: E712  (the reference's own spelling)
        x = x / (x.norm(dim=2, keepdim=True) + 1e-9)
        total = x.sum(dim=1).pow(2).sum(dim=1)              # || sum_i x^_i ||^2     [B]
        diag = x.pow(2).sum(dim=(1, 2))                     # sum_i || x^_i ||^2     [B]
        return ((total - diag) / float(n_frames * n_frames)).mean()

    def forward(self, x: Tensor, video_representation: Tensor, mask=None, visualize_attention=None,
                pen_met: str = "entropy"):
        # `visualize_attention` would make the reference unpack a 2-tuple into (out, attention) and crash a line
        # later (simnet_pretrain.py:75-78); no caller passes it, and it is ignored here.
        logits, hidden = self.encoder(x, mask, model_score=True)                                      # :77
        if not hidden.is_cuda:
            raise RuntimeError("PretrainModel runs on the MI355X HIP kernels only (HIP tensors)")
        if logits.size(2) != 1:
            raise RuntimeError("PretrainModel needs num_classes == 1 (one score per frame)")
        losses = _PretrainHead.apply(hidden, logits, video_representation.to(hidden.device), mask if isinstance(mask, Tensor) else None,
                                     self.video_transform.weight, self.video_transform.bias, self.sharpening_t,
                                     pen_met == "entropy")
        return losses[0], losses[1], losses[2]

    def forward_packed(self, x: Tensor, video_representation: Tensor, lengths, pen_met: str = "entropy", ref_len=None):
        """``forward`` on a RAGGED batch without padding: x [sum(lengths), 1024] = the videos' frames concatenated
        (``data.collate_fn_pretrain_packed``), video_representation [B, 512].  Returns the same triple (distillation,
        centering, repelling).  The encoder is ``SimNet.forward_packed_train`` (it follows ``set_train_dtype``; its packed
        attention is exact fp32 unless ``self.encoder.set_train_dtype(..., packed_attention=True)`` opted in), the head below it ``_PretrainHeadPacked``, exact fp32 in every mode; no padded row is
        computed in either, forward or backward.

        Equality with the padded step: the reference pads a batch to its longest video with the 1000.0 sentinel and masks
        (pretrain.py:57); masked frames get softmax weight 0 and zero rows in the repelling loss, but stay in two
        denominators - the centering mean over frames (``mean(dim=1)``) and the [T,T] mean of the repelling loss.  ``ref_len``
        is that padded width.  With ``ref_len=None`` (= ``max(lengths)``) the three losses and every gradient equal those of
        ``forward(x_padded, video_representation, mask)`` on the padded batch of the same videos, up to fp32 rounding.  A
        larger ``ref_len`` reproduces a batch padded wider (and, held fixed, makes a video's terms independent of its
        batch-mates); a smaller one raises."""
        lengths = [int(t) for t in lengths]
        if not lengths or min(lengths) <= 0:
            raise RuntimeError("lengths must be positive, got %r" % (lengths,))
        if ref_len is None:
            ref_len = max(lengths)
        if int(ref_len) < max(lengths):
            raise RuntimeError("ref_len=%d is below max(lengths)=%d (it is the width the batch would have been padded to)"
                               % (int(ref_len), max(lengths)))
        if x.dim() != 2 or x.size(0) != sum(lengths) or x.size(1) != self.encoder.in_features:
            raise RuntimeError("expected x of shape [sum(lengths)=%d, %d], got %s" % (sum(lengths), self.encoder.in_features, tuple(x.shape)))
        if video_representation.dim() != 2 or video_representation.size(0) != len(lengths):
            raise RuntimeError("expected video_representation of shape [%d, F], got %s" % (len(lengths), tuple(video_representation.shape)))
        if not x.is_cuda:
            raise RuntimeError("PretrainModel runs on the MI355X HIP kernels only (HIP tensors)")
        with torch.cuda.device(x.device):
            lengths_dev = _device_lengths(lengths, x.device)                # before the encoder: nothing to wait for mid-step
        logits, hidden = self.encoder.forward_packed_train(x, lengths)
        if logits.size(1) != 1:
            raise RuntimeError("PretrainModel needs num_classes == 1 (one score per frame)")
        losses = _PretrainHeadPacked.apply(hidden, logits, video_representation.to(hidden.device), lengths, int(ref_len),
                                           self.video_transform.weight, self.video_transform.bias, self.sharpening_t,
                                           pen_met == "entropy", lengths_dev)
        return losses[0], losses[1], losses[2]
