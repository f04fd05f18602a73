"""GoogLeNet pool5 frame features on the GPU: frames in, ``[T, 1024]`` out (C ABI: ``include/features/vs_features.h``).

Drop-in for the reference's ``get_google_net_features`` (``src/data/preprocess/feature_extraction.py:10-42``) over its
``models.GoogleNet`` (``src/data/preprocess/models.py:10-37``): torchvision's ``googlenet(aux_logits=False)`` without ``dropout``
and ``fc``, as an ``nn.Sequential`` - so ``transform_input`` (which lives in ``GoogLeNet.forward``) is never applied, and is not
applied here either.

BatchNorm statistics: the reference never calls ``.eval()``, so its BatchNorm layers would normalise every batch by that batch's
own statistics - a frame's features would depend on the frames it is batched with.  That is a defect and is NOT reproduced: this
module always uses the running statistics, which is what every published ``google_pool5`` feature set uses.  ``train()`` does not
change that.

The reference's ``transforms.Resize`` in front of the network: ``resize_frames`` on the host through PIL (the default), or
``resize_frames_device`` / ``extract(frames, size=...)`` on the device, bit-equal to it (C ABI: ``include/features/vs_resize.h``).

There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import torch
from torch import Tensor, nn

from . import _lib
from ._call import on_stream, scratch

# Inception(in, c1, c3r, c3, c5r, c5, pp); "branch3" is 3x3, not 5x5 (torchvision's known deviation)
INCEPTIONS = OrderedDict([
    ("inception3a", (192, 64, 96, 128, 16, 32, 32)), ("inception3b", (256, 128, 128, 192, 32, 96, 64)),
    ("inception4a", (480, 192, 96, 208, 16, 48, 64)), ("inception4b", (512, 160, 112, 224, 24, 64, 64)),
    ("inception4c", (512, 128, 128, 256, 24, 64, 64)), ("inception4d", (512, 112, 144, 288, 32, 64, 64)),
    ("inception4e", (528, 256, 160, 320, 32, 128, 128)), ("inception5a", (832, 256, 160, 320, 32, 128, 128)),
    ("inception5b", (832, 384, 192, 384, 48, 128, 128))])
# the reference's nn.Sequential(*children()[:-2]): index -> torchvision name (its own state_dict() says model.<i>.…)
SEQUENTIAL_NAMES = ("conv1", "maxpool1", "conv2", "conv3", "maxpool2", "inception3a", "inception3b", "maxpool3", "inception4a",
                    "inception4b", "inception4c", "inception4d", "inception4e", "maxpool4", "inception5a", "inception5b", "avgpool")
BN_EPS = 0.001


def conv_table():
    """[(torchvision prefix, cout, cin, k, stride, pad)] of the 57 convs, in the order of ``vs_cnn_params``"""
    t = [("conv1", 64, 3, 7, 2, 3), ("conv2", 64, 64, 1, 1, 0), ("conv3", 192, 64, 3, 1, 1)]
    for name, (cin, c1, c3r, c3, c5r, c5, pp) in INCEPTIONS.items():
        t += [(name + ".branch1", c1, cin, 1, 1, 0), (name + ".branch2.0", c3r, cin, 1, 1, 0), (name + ".branch2.1", c3, c3r, 3, 1, 1),
              (name + ".branch3.0", c5r, cin, 1, 1, 0), (name + ".branch3.1", c5, c5r, 3, 1, 1), (name + ".branch4.1", pp, cin, 1, 1, 0)]
    return t


def state_dict_shapes():
    """{torchvision key: shape} of every parameter and buffer, in ``state_dict()`` order"""
    out = OrderedDict()
    for prefix, cout, cin, k, _, _ in conv_table():
        out[prefix + ".conv.weight"] = (cout, cin, k, k)
        for f in ("weight", "bias", "running_mean", "running_var"):
            out[prefix + ".bn." + f] = (cout,)
        out[prefix + ".bn.num_batches_tracked"] = ()
    return out


def make_state_dict(seed: int):
    """Seeded random weights and statistics under torchvision's names (tests, smoke-style checks, the bench): He-scaled convs,
    gamma and running_var in [0.5, 1.5], small beta and running_mean - activations keep their scale through the 22 layers."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for key, shape in state_dict_shapes().items():
        if key.endswith("conv.weight"):
            sd[key] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif key.endswith("bn.weight") or key.endswith("running_var"):
            sd[key] = 0.5 + torch.rand(shape, generator=g)
        elif key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(1, dtype=torch.long)
        else:
            sd[key] = 0.1 * torch.randn(shape, generator=g)
    return sd


def strip_torchvision_head(sd):
    """A ``torchvision.models.googlenet`` checkpoint without what the reference cuts off: ``fc.*``, ``aux1.*``, ``aux2.*``"""
    return OrderedDict((k, v) for k, v in sd.items() if k.split(".")[0] not in ("fc", "aux1", "aux2"))


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


class _BasicConv2d(nn.Module):
    """holds conv.weight and bn.{weight, bias, running_mean, running_var, num_batches_tracked} under torchvision's names"""

    def __init__(self, cin, cout, k, stride, pad):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=pad, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=BN_EPS)


class _Inception(nn.Module):
    def __init__(self, cin, c1, c3r, c3, c5r, c5, pp):
        super().__init__()
        self.branch1 = _BasicConv2d(cin, c1, 1, 1, 0)
        self.branch2 = nn.Sequential(_BasicConv2d(cin, c3r, 1, 1, 0), _BasicConv2d(c3r, c3, 3, 1, 1))
        self.branch3 = nn.Sequential(_BasicConv2d(cin, c5r, 1, 1, 0), _BasicConv2d(c5r, c5, 3, 1, 1))
        self.branch4 = nn.Sequential(nn.MaxPool2d(3, stride=1, padding=1, ceil_mode=True), _BasicConv2d(cin, pp, 1, 1, 0))


class _PackedCnn:
    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        try:
            if self.handle:
                _lib.load().vs_cnn_free(self.handle)
                self.handle = None
        except Exception:
            pass


class GoogLeNetFeatures(nn.Module):
    """torchvision's GoogLeNet up to ``avgpool`` on the HIP kernels: ``forward(x)`` for the normalised ``[N, 3, H, W]`` float32
    tensor the reference's model receives, ``extract(frames)`` for decoded ``[N, H, W, 3]`` uint8 frames (the reference's
    ``ToTensor`` + ``Normalize`` run inside conv1's gather).  Both return ``[N, 1024]`` float32 on the device, run without
    autograd, and a frame's features are bit-identical whatever batch or chunk it is computed in.

    Parameters and buffers carry torchvision's names, so ``load_state_dict(strip_torchvision_head(checkpoint))`` loads a
    ``torchvision.models.googlenet`` checkpoint; the reference's own ``model.<i>.…`` names are accepted too.

    BatchNorm always uses the running statistics (see the module docstring): ``train()`` does not switch to batch statistics.
    Long inputs run in chunks of ``max_batch`` frames, so the workspace does not grow with the video."""

    def __init__(self, max_batch: int = 64):
        super().__init__()
        if max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        self.max_batch = int(max_batch)
        self.conv1 = _BasicConv2d(3, 64, 7, 2, 3)
        self.maxpool1 = nn.MaxPool2d(3, stride=2, ceil_mode=True)
        self.conv2 = _BasicConv2d(64, 64, 1, 1, 0)
        self.conv3 = _BasicConv2d(64, 192, 3, 1, 1)
        self.maxpool2 = nn.MaxPool2d(3, stride=2, ceil_mode=True)
        for name, cfg in INCEPTIONS.items():
            if name == "inception4a":
                self.maxpool3 = nn.MaxPool2d(3, stride=2, ceil_mode=True)
            if name == "inception5a":
                self.maxpool4 = nn.MaxPool2d(2, stride=2, ceil_mode=True)
            setattr(self, name, _Inception(*cfg))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self._packed = None
        self._packed_key = None

    def load_state_dict(self, state_dict, *args, **kwargs):
        return super().load_state_dict(from_sequential_names(state_dict), *args, **kwargs)

    def _tensors(self):
        for prefix, *_ in conv_table():
            m = self.get_submodule(prefix)
            yield from (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)

    def _packed_weights(self, device) -> _PackedCnn:
        """vs_cnn_weights* for the current values; re-packed whenever a parameter or statistic was written (``load_state_dict``,
        ``.to()``, an optimiser) - detected by (data_ptr, _version), as SimNet does."""
        tensors = list(self._tensors())
        key = (device,) + tuple((t.data_ptr(), t._version) for t in tensors)
        if self._packed is not None and key == self._packed_key:
            return self._packed
        for t in tensors:
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("GoogLeNetFeatures: parameters must be contiguous float32 on the input's device (%s)" % device)
        P = _lib.CnnParams()
        it = iter(tensors)
        for i in range(_lib.VS_CNN_NUM_CONVS):
            for f in ("weight", "gamma", "beta", "running_mean", "running_var"):
                setattr(P.conv[i], f, next(it).data_ptr())
        handle = C.c_void_p()
        with on_stream(device) as stream:
            _lib.check(_lib.load().vs_cnn_pack(C.byref(P), stream, C.byref(handle)))
        self._packed, self._packed_key = _PackedCnn(handle), key
        return self._packed

    def _run(self, x: Tensor, kind: int, n: int, h: int, w: int) -> Tensor:
        lib = _lib.load()
        dev = x.device
        packed = self._packed_weights(dev)
        out = torch.empty((n, _lib.VS_CNN_FEATURES), dtype=torch.float32, device=dev)
        step = min(n, self.max_batch)
        need = lib.vs_cnn_workspace_bytes(step, h, w)
        with on_stream(dev) as stream:
            if need == 0:       # vs_last_error() says why (a frame below the smallest accepted side, a batch too large)
                _lib.check(_lib.VS_ERR_INVALID)
            ws = scratch(need, dev, floor=256)
            for at in range(0, n, step):
                chunk = x.narrow(0, at, min(step, n - at))
                _lib.check(lib.vs_cnn_forward(packed.handle, chunk.data_ptr(), kind, chunk.size(0), h, w, out[at:].data_ptr(),
                                              ws.data_ptr(), ws.numel(), stream))
        return out

    @staticmethod
    def _check_hip(x: Tensor) -> None:
        if not x.is_cuda:
            raise RuntimeError("GoogLeNetFeatures runs on the MI355X HIP kernels only: move the module and its input to a HIP "
                               "device (there is no CPU path for the feature extractor)")

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        """``x``: ``[N, 3, H, W]`` float32, normalised as the reference's transform does -> ``[N, 1024]``"""
        self._check_hip(x)
        if x.dim() != 4 or x.size(1) != 3 or x.dtype != torch.float32:
            raise ValueError("expected a float32 [N, 3, H, W] tensor, got %s %s" % (x.dtype, tuple(x.shape)))
        if x.size(0) == 0:
            return x.new_empty((0, _lib.VS_CNN_FEATURES))
        x = x.contiguous()
        return self._run(x, _lib.VS_CNN_INPUT_F32_NCHW, x.size(0), x.size(2), x.size(3))

    @torch.no_grad()
    def extract(self, frames: Tensor, size=None, bgr: bool = False) -> Tensor:
        """``frames``: ``[N, H, W, 3]`` uint8 RGB on the device -> ``[N, 1024]``; x / 255, - mean, / std happen in conv1.
        ``size`` (an int for the shorter side, or (h, w)) resizes on the device first, bit-equal to the reference's
        ``transforms.Resize(size)`` on PIL images: each chunk of ``max_batch`` frames is resized into scratch and fed to conv1,
        so the resized video is never held whole.  ``bgr=True`` takes decoded OpenCV frames (B, G, R)."""
        self._check_hip(frames)
        if frames.dim() != 4 or frames.size(3) != 3 or frames.dtype != torch.uint8:
            raise ValueError("expected a uint8 [N, H, W, 3] tensor, got %s %s" % (frames.dtype, tuple(frames.shape)))
        if frames.size(0) == 0:
            return torch.empty((0, _lib.VS_CNN_FEATURES), dtype=torch.float32, device=frames.device)
        frames = frames.contiguous()
        if size is None and not bgr:
            return self._run(frames, _lib.VS_CNN_INPUT_U8_NHWC, frames.size(0), frames.size(1), frames.size(2))
        return self._run_resized(frames, size, bgr)

    def _run_resized(self, frames: Tensor, size, bgr: bool) -> Tensor:
        """``_run`` with the device resize (and / or the R/B swap) in front of conv1, chunk by chunk"""
        lib = _lib.load()
        dev = frames.device
        n, h, w = frames.size(0), frames.size(1), frames.size(2)
        oh, ow = (h, w) if size is None else resize_output_size(h, w, size)
        plan = _resize_plan(dev, h, w, oh, ow)
        packed = self._packed_weights(dev)
        out = torch.empty((n, _lib.VS_CNN_FEATURES), dtype=torch.float32, device=dev)
        step = min(n, self.max_batch)
        need = lib.vs_cnn_workspace_bytes(step, oh, ow)
        flags = _lib.VS_RESIZE_SWAP_RB if bgr else 0
        with on_stream(dev) as stream:
            if need == 0:
                _lib.check(_lib.VS_ERR_INVALID)
            ws = scratch(need, dev, floor=256)
            small = torch.empty((step, oh, ow, 3), dtype=torch.uint8, device=dev)
            rws = scratch(lib.vs_resize_workspace_bytes(plan.handle, step), dev)
            for at in range(0, n, step):
                chunk = frames.narrow(0, at, min(step, n - at))
                _lib.check(lib.vs_resize_run(plan.handle, chunk.data_ptr(), chunk.size(0), flags, small.data_ptr(),
                                             rws.data_ptr() if rws.numel() else None, rws.numel(), stream))
                _lib.check(lib.vs_cnn_forward(packed.handle, small.data_ptr(), _lib.VS_CNN_INPUT_U8_NHWC, chunk.size(0), oh, ow,
                                              out[at:].data_ptr(), ws.data_ptr(), ws.numel(), stream))
        return out


def resize_frames(video, size):
    """The reference's ``transforms.Resize(size)`` on the host, frame by frame through PIL: an int scales the shorter side
    (bilinear, as torchvision does for PIL images), a pair is (h, w).  [T, H, W, 3] uint8 numpy in and out."""
    import numpy as np
    from PIL import Image
    t, h, w = video.shape[:3]
    if isinstance(size, int):
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = size, int(size * long / short)
        ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
    else:
        oh, ow = size
    if (oh, ow) == (h, w):
        return np.ascontiguousarray(video)
    out = np.empty((t, oh, ow, 3), dtype=np.uint8)
    for i in range(t):
        out[i] = np.asarray(Image.fromarray(video[i]).resize((ow, oh), Image.BILINEAR))
    return out


def resize_output_size(h: int, w: int, size):
    """(oh, ow) of ``transforms.Resize(size)`` for an ``h x w`` image: an int scales the shorter side to ``size`` and the longer
    to ``int(size * long / short)`` (``w <= h`` counts as "w is shorter"), a pair is (h, w).  The rule inside ``resize_frames``,
    computed by the library (``vs_resize_output_size``)."""
    if isinstance(size, int):
        oh, ow = C.c_int32(), C.c_int32()
        _lib.check(_lib.load().vs_resize_output_size(int(h), int(w), size, C.byref(oh), C.byref(ow)))
        return oh.value, ow.value
    oh, ow = size
    return int(oh), int(ow)


class _ResizePlan:
    """vs_resize_plan* of one (device, geometry): the coefficient tables on the device and the tile the host chose"""

    def __init__(self, device, h, w, oh, ow):
        self.handle = C.c_void_p()
        with on_stream(device) as stream:
            _lib.check(_lib.load().vs_resize_plan_create(h, w, oh, ow, stream, C.byref(self.handle)))
        path, th, tw = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.load().vs_resize_plan_describe(self.handle, C.byref(path), C.byref(th), C.byref(tw)))
        self.path, self.tile = path.value, (th.value, tw.value)

    def __del__(self):
        try:
            if self.handle:
                _lib.load().vs_resize_plan_free(self.handle)
                self.handle = None
        except Exception:
            pass


_RESIZE_PLANS = {}


def _resize_plan(device, h, w, oh, ow) -> _ResizePlan:
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), h, w, oh, ow)
    plan = _RESIZE_PLANS.get(key)
    if plan is None:
        plan = _RESIZE_PLANS[key] = _ResizePlan(device, h, w, oh, ow)
    return plan


def resize_plan_path(device, h: int, w: int, oh: int, ow: int):
    """(path, (tile_oh, tile_ow)) the cached plan of this geometry chose: ``_lib.VS_RESIZE_PATH_FUSED`` for the default tile,
    ``_lib.VS_RESIZE_PATH_SMALL_TILE`` where its input rows or columns would not fit the LDS staging"""
    plan = _resize_plan(device, h, w, oh, ow)
    return plan.path, plan.tile


@torch.no_grad()
def resize_frames_device(frames: Tensor, size, *, bgr: bool = False) -> Tensor:
    """``resize_frames`` on the device: uint8 ``[N, H, W, 3]`` on a HIP device -> uint8 ``[N, oh, ow, 3]``, bit-equal to
    ``PIL.Image.resize((ow, oh), Image.BILINEAR)`` frame by frame (C ABI: ``include/features/vs_resize.h``).  ``bgr=True`` swaps
    R and B on the way (decoded OpenCV frames).  With equal sizes and ``bgr=False`` the input itself is returned.  Plans (the
    coefficient tables) are cached per (device, geometry).  There is no CPU path: a CPU tensor raises."""
    if not frames.is_cuda:
        raise RuntimeError("resize_frames_device runs on the MI355X HIP kernel only: move the frames to a HIP device "
                           "(there is no CPU path; resize_frames is the host form)")
    if frames.dim() != 4 or frames.size(3) != 3 or frames.dtype != torch.uint8:
        raise ValueError("expected a uint8 [N, H, W, 3] tensor, got %s %s" % (frames.dtype, tuple(frames.shape)))
    n, h, w = frames.size(0), frames.size(1), frames.size(2)
    oh, ow = resize_output_size(h, w, size)
    if (oh, ow) == (h, w) and not bgr:
        return frames
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=frames.device)
    if n == 0:
        return out
    frames = frames.contiguous()
    lib = _lib.load()
    plan = _resize_plan(frames.device, h, w, oh, ow)
    with on_stream(frames.device) as stream:
        ws = scratch(lib.vs_resize_workspace_bytes(plan.handle, n), frames.device)
        _lib.check(lib.vs_resize_run(plan.handle, frames.data_ptr(), n, _lib.VS_RESIZE_SWAP_RB if bgr else 0, out.data_ptr(),
                                     ws.data_ptr() if ws.numel() else None, ws.numel(), stream))
    return out


def get_google_net_features(video, size=224, *, model: GoogLeNetFeatures = None, weights=None, device="cuda", resize="host"):
    """Drop-in for the reference's function: ``video`` numpy uint8 ``[T, H, W, 3]`` -> numpy float32 ``[T, 1024]``.  With
    ``resize="host"`` (the default) the resize runs on the host exactly as in the reference (``size=None`` skips it) and
    everything after it on the device; ``resize="device"`` uploads the raw frames in chunks of ``model.max_batch`` and resizes
    them there, to the same bytes.  Pretrained weights
    are never fetched: pass ``model=`` (a ``GoogLeNetFeatures`` on a HIP device) or ``weights=`` (a path for ``torch.load`` or a
    state dict, a torchvision ``googlenet`` checkpoint or the reference's ``model.<i>`` form)."""
    import numpy as np
    if resize not in ("host", "device"):
        raise ValueError("resize must be 'host' or 'device', got %r" % (resize,))
    if model is None:
        if weights is None:
            raise ValueError("get_google_net_features needs model= or weights= (a torchvision googlenet checkpoint): "
                             "this package never downloads pretrained weights")
        sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") else weights
        model = GoogLeNetFeatures()
        model.load_state_dict(strip_torchvision_head(from_sequential_names(sd)), strict=True)
        model = model.to(device)
    video = np.asarray(video)
    if video.ndim != 4 or video.shape[3] != 3 or video.dtype != np.uint8:
        raise ValueError("expected a uint8 [T, H, W, 3] array, got %s %s" % (video.dtype, video.shape))
    dev = next(model.parameters()).device
    if resize == "device" and size is not None:
        out = np.empty((video.shape[0], _lib.VS_CNN_FEATURES), dtype=np.float32)
        for at in range(0, video.shape[0], model.max_batch):
            raw = torch.from_numpy(np.ascontiguousarray(video[at:at + model.max_batch])).to(dev)
            out[at:at + raw.size(0)] = model.extract(raw, size=size).cpu().numpy()
        return out
    if size is not None:
        video = resize_frames(video, size)
    frames = torch.from_numpy(np.ascontiguousarray(video)).to(dev)
    return model.extract(frames).cpu().numpy()
