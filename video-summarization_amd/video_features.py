"""R3D-18 video-level features on the GPU: the frames of a video in, ``[512]`` out (C ABI: ``include/features/vs_video_features.h``).

Drop-in for the reference's ``get_video_feature`` (``src/data/preprocess/feature_extraction.py:45-76``) over its ``models.R3D18``
(``src/data/preprocess/models.py:40-66``): torchvision's ``r3d_18`` up to and including ``avgpool`` as an ``nn.Sequential``, then
``flatten(1)``.  The vector is the target that pretraining distils against (``PretrainModel.video_transform`` is
``Linear(d_model, 512)``).

BatchNorm statistics: the reference never calls ``.eval()``, so its BatchNorm3d layers would normalise every channel by this one
video's own statistics.  That is a defect and is NOT reproduced: this module always uses the running statistics (eps 1e-5), as
``features.GoogLeNetFeatures`` does.  ``train()`` does not change that.

Pretrained weights are never fetched: ``weights=`` or ``model=`` is required, and every number this project states about the
module was taken on seeded random weights (``make_state_dict``), not on a Kinetics checkpoint.

The whole video runs as one clip, as in the reference; the workspace grows with it (about 1 GB for 320 frames of 122 x 122).
There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import torch
from torch import Tensor, nn

from . import _lib
from ._call import on_stream, scratch
from .features import resize_frames, resize_frames_device

# the reference's nn.Sequential(*children()[:-1]): index -> torchvision name (its own state_dict() says model.<i>.…)
SEQUENTIAL_NAMES = ("stem", "layer1", "layer2", "layer3", "layer4", "avgpool")
PLANES = (64, 128, 256, 512)
BN_EPS = 1e-5
FEATURES = 512


def conv_table():
    """[(torchvision prefix, cout, cin, (kt, ks), (stride_t, stride_s), (pad_t, pad_s))] of the 20 convs in execution order, the
    order of ``vs_r3d_params``: the stem, then per block conv1, downsample (first block of layer2..4), conv2.  ``prefix + ".0"``
    is the conv, ``prefix + ".1"`` its BatchNorm3d."""
    t = [("stem", 64, 3, (3, 7), (1, 2), (1, 3))]
    cin = 64
    for layer, planes in enumerate(PLANES, 1):
        for block in range(2):
            s = 2 if layer > 1 and block == 0 else 1
            p = "layer%d.%d" % (layer, block)
            t.append((p + ".conv1", planes, cin, (3, 3), (s, s), (1, 1)))
            if s == 2:
                t.append((p + ".downsample", planes, cin, (1, 1), (2, 2), (0, 0)))
            t.append((p + ".conv2", planes, planes, (3, 3), (1, 1), (1, 1)))
            cin = planes
    return t


def state_dict_shapes():
    """{torchvision key: shape} of every parameter and buffer, in ``state_dict()`` order (a block registers conv1, conv2, downsample)"""
    table = {row[0]: row for row in conv_table()}
    order = ["stem"] + [p for layer in range(1, 5) for block in range(2)
                        for p in ["layer%d.%d.%s" % (layer, block, c) for c in ("conv1", "conv2", "downsample")] if p in table]
    out = OrderedDict()
    for prefix in order:
        _, cout, cin, (kt, ks), _, _ = table[prefix]
        out[prefix + ".0.weight"] = (cout, cin, kt, ks, ks)
        for f in ("weight", "bias", "running_mean", "running_var"):
            out[prefix + ".1." + f] = (cout,)
        out[prefix + ".1.num_batches_tracked"] = ()
    return out


def make_state_dict(seed: int):
    """Seeded random weights and statistics under torchvision's names (tests, the bench): He-scaled convs, gamma and running_var
    in [0.5, 1.5], small beta and running_mean, as ``features.make_state_dict``"""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for key, shape in state_dict_shapes().items():
        if key.endswith(".0.weight"):
            sd[key] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3] * shape[4])) ** 0.5
        elif key.endswith(".1.weight") or key.endswith("running_var"):
            sd[key] = 0.5 + torch.rand(shape, generator=g)
        elif key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(1, dtype=torch.long)
        else:
            sd[key] = 0.1 * torch.randn(shape, generator=g)
    return sd


def strip_torchvision_head(sd):
    """A ``torchvision.models.video.r3d_18`` checkpoint without what the reference cuts off: ``fc.*``"""
    return OrderedDict((k, v) for k, v in sd.items() if k.split(".")[0] != "fc")


def from_sequential_names(sd):
    """The reference's ``model.<i>.…`` keys -> torchvision's names; other keys pass unchanged"""
    out = OrderedDict()
    for k, v in sd.items():
        parts = k.split(".")
        if parts[0] == "model" and len(parts) > 2 and parts[1].isdigit() and int(parts[1]) < len(SEQUENTIAL_NAMES):
            k = ".".join([SEQUENTIAL_NAMES[int(parts[1])]] + parts[2:])
        out[k] = v
    return out


def to_sequential_names(sd):
    """torchvision's names -> the reference's ``model.<i>.…`` keys"""
    index = {name: i for i, name in enumerate(SEQUENTIAL_NAMES)}
    return OrderedDict(("model.%d.%s" % (index[k.split(".")[0]], k.split(".", 1)[1]), v) for k, v in sd.items())


def _conv_bn(cin, cout, k, stride, pad, relu):
    kt, ks = k
    layers = [nn.Conv3d(cin, cout, (kt, ks, ks), stride=(stride[0], stride[1], stride[1]), padding=(pad[0], pad[1], pad[1]), bias=False),
              nn.BatchNorm3d(cout, eps=BN_EPS)]
    return nn.Sequential(*(layers + ([nn.ReLU(inplace=True)] if relu else [])))


class _BasicBlock(nn.Module):
    """holds conv1.{0,1}, conv2.{0,1} and downsample.{0,1} under torchvision's names, registered in torchvision's order"""

    def __init__(self, cin, planes, stride):
        super().__init__()
        self.conv1 = _conv_bn(cin, planes, (3, 3), (stride, stride), (1, 1), True)
        self.conv2 = _conv_bn(planes, planes, (3, 3), (1, 1), (1, 1), False)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = _conv_bn(cin, planes, (1, 1), (2, 2), (0, 0), False) if stride == 2 else None


class _PackedR3d:
    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        try:
            if self.handle:
                _lib.load().vs_r3d_free(self.handle)
                self.handle = None
        except Exception:
            pass


class R3D18Features(nn.Module):
    """torchvision's ``r3d_18`` up to ``avgpool`` on the HIP kernels: ``forward(x)`` for the normalised ``[N, 3, T, H, W]`` float32
    tensor the reference's model receives, ``extract(frames)`` for decoded uint8 frames ``[T, H, W, 3]`` or ``[N, T, H, W, 3]``
    (the reference's ``ToTensor`` + ``Normalize`` run inside the stem's gather, and the frame stack is read as it lies: nothing is
    permuted).  Both return ``[N, 512]`` float32 on the device, run without autograd, and a video's feature is bit-identical
    whatever batch it is computed in.

    Parameters and buffers carry torchvision's names, so ``load_state_dict(strip_torchvision_head(checkpoint), strict=True)``
    loads a ``torchvision.models.video.r3d_18`` checkpoint; the reference's own ``model.<i>.…`` names are accepted too.

    BatchNorm always uses the running statistics (see the module docstring): ``train()`` does not switch to batch statistics."""

    def __init__(self):
        super().__init__()
        self.stem = _conv_bn(3, 64, (3, 7), (1, 2), (1, 3), True)
        cin = 64
        for layer, planes in enumerate(PLANES, 1):
            setattr(self, "layer%d" % layer, nn.Sequential(_BasicBlock(cin, planes, 2 if layer > 1 else 1), _BasicBlock(planes, planes, 1)))
            cin = planes
        self.avgpool = nn.AdaptiveAvgPool3d(1)
        self._packed = None
        self._packed_key = None

    def load_state_dict(self, state_dict, *args, **kwargs):
        return super().load_state_dict(from_sequential_names(state_dict), *args, **kwargs)

    def _tensors(self):
        for prefix, *_ in conv_table():
            m = self.get_submodule(prefix)
            yield from (m[0].weight, m[1].weight, m[1].bias, m[1].running_mean, m[1].running_var)

    def _packed_weights(self, device) -> _PackedR3d:
        """vs_r3d_weights* for the current values; re-packed whenever a parameter or statistic was written (``load_state_dict``,
        ``.to()``, an in-place change) - detected by (data_ptr, _version), as ``GoogLeNetFeatures`` does."""
        tensors = list(self._tensors())
        key = (device,) + tuple((t.data_ptr(), t._version) for t in tensors)
        if self._packed is not None and key == self._packed_key:
            return self._packed
        for t in tensors:
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("R3D18Features: parameters must be contiguous float32 on the input's device (%s)" % device)
        P = _lib.R3dParams()
        it = iter(tensors)
        for i in range(_lib.VS_R3D_NUM_CONVS):
            for f in ("weight", "gamma", "beta", "running_mean", "running_var"):
                setattr(P.conv[i], f, next(it).data_ptr())
        handle = C.c_void_p()
        with on_stream(device) as stream:
            _lib.check(_lib.load().vs_r3d_pack(C.byref(P), stream, C.byref(handle)))
        self._packed, self._packed_key = _PackedR3d(handle), key
        return self._packed

    def _run(self, x: Tensor, kind: int, n: int, t: int, h: int, w: int) -> Tensor:
        lib = _lib.load()
        dev = x.device
        packed = self._packed_weights(dev)
        out = torch.empty((n, FEATURES), dtype=torch.float32, device=dev)
        need = lib.vs_r3d_workspace_bytes(n, t, h, w)
        with on_stream(dev) as stream:
            if need == 0:       # vs_last_error() says why (a batch too large)
                _lib.check(_lib.VS_ERR_INVALID)
            ws = scratch(need, dev, floor=256)
            _lib.check(lib.vs_r3d_forward(packed.handle, x.data_ptr(), kind, n, t, h, w, out.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return out

    @staticmethod
    def _check_hip(x: Tensor) -> None:
        if not x.is_cuda:
            raise RuntimeError("R3D18Features runs on the MI355X HIP kernels only: move the module and its input to a HIP "
                               "device (there is no CPU path for the feature extractor)")

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        """``x``: ``[N, 3, T, H, W]`` float32, normalised as the reference's transform does -> ``[N, 512]``"""
        self._check_hip(x)
        if x.dim() != 5 or x.size(1) != 3 or x.dtype != torch.float32:
            raise ValueError("expected a float32 [N, 3, T, H, W] tensor, got %s %s" % (x.dtype, tuple(x.shape)))
        if x.numel() == 0:
            raise ValueError("expected at least one video, frame and pixel, got %s" % (tuple(x.shape),))
        x = x.contiguous()
        return self._run(x, _lib.VS_CNN3D_INPUT_F32_NCDHW, x.size(0), x.size(2), x.size(3), x.size(4))

    @torch.no_grad()
    def extract(self, frames: Tensor, size=None, bgr: bool = False) -> Tensor:
        """``frames``: ``[T, H, W, 3]`` (one video) or ``[N, T, H, W, 3]`` uint8 RGB on the device -> ``[N, 512]``; x / 255, - mean,
        / std happen in the stem.  ``size`` (an int for the shorter side, or (h, w)) resizes on the device first through
        ``resize_frames_device``, bit-equal to the reference's ``transforms.Resize(size)`` on PIL images.  ``bgr=True`` takes
        decoded OpenCV frames (B, G, R)."""
        self._check_hip(frames)
        if frames.dim() == 4:
            frames = frames.unsqueeze(0)
        if frames.dim() != 5 or frames.size(4) != 3 or frames.dtype != torch.uint8:
            raise ValueError("expected a uint8 [T, H, W, 3] or [N, T, H, W, 3] tensor, got %s %s" % (frames.dtype, tuple(frames.shape)))
        if frames.numel() == 0:
            raise ValueError("expected at least one video, frame and pixel, got %s" % (tuple(frames.shape),))
        frames = frames.contiguous()
        n, t = frames.size(0), frames.size(1)
        if size is not None or bgr:
            flat = frames.view(n * t, frames.size(2), frames.size(3), 3)
            flat = resize_frames_device(flat, (frames.size(2), frames.size(3)) if size is None else size, bgr=bgr)
            frames = flat.view(n, t, flat.size(1), flat.size(2), 3)
        return self._run(frames, _lib.VS_CNN3D_INPUT_U8_NDHWC, n, t, frames.size(2), frames.size(3))


def get_video_feature(video, size=112, *, model: R3D18Features = None, weights=None, device="cuda", resize="host"):
    """Drop-in for the reference's function: ``video`` numpy uint8 ``[T, H, W, 3]`` -> numpy float32 ``[512]``.  With
    ``resize="host"`` (the default) the resize runs on the host through PIL exactly as in the reference (``size=None`` skips it)
    and everything after it on the device; ``resize="device"`` uploads the raw frames and resizes them there, to the same bytes.
    Pretrained weights are never fetched: pass ``model=`` (an ``R3D18Features`` on a HIP device) or ``weights=`` (a path for
    ``torch.load`` or a state dict, a torchvision ``r3d_18`` checkpoint or the reference's ``model.<i>`` form)."""
    import numpy as np
    if resize not in ("host", "device"):
        raise ValueError("resize must be 'host' or 'device', got %r" % (resize,))
    if model is None:
        if weights is None:
            raise ValueError("get_video_feature needs model= or weights= (a torchvision r3d_18 checkpoint): "
                             "this package never downloads pretrained weights")
        sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") else weights
        model = R3D18Features()
        model.load_state_dict(strip_torchvision_head(from_sequential_names(sd)), strict=True)
        model = model.to(device)
    video = np.asarray(video)
    if video.ndim != 4 or video.shape[3] != 3 or video.dtype != np.uint8:
        raise ValueError("expected a uint8 [T, H, W, 3] array, got %s %s" % (video.dtype, video.shape))
    dev = next(model.parameters()).device
    if resize == "device" and size is not None:
        return model.extract(torch.from_numpy(np.ascontiguousarray(video)).to(dev), size=size)[0].cpu().numpy()
    if size is not None:
        video = resize_frames(video, size)
    return model.extract(torch.from_numpy(np.ascontiguousarray(video)).to(dev))[0].cpu().numpy()
