"""The oracle of the GoogLeNet pool5 front end: our own restatement of torchvision's ``googlenet(aux_logits=False)`` without
``dropout`` and ``fc`` (the reference's ``models.GoogleNet``) in plain torch functions, in whatever dtype the input has - float64
as the oracle, float32 to measure what fp32 arithmetic itself costs.  BatchNorm in eval mode (running statistics), eps 0.001;
``transform_input`` is not applied (the reference's ``nn.Sequential`` bypasses it).  Runs on the CPU or on a device."""
import torch
import torch.nn.functional as F

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BLOCKS = ("inception3a", "inception3b", None, "inception4a", "inception4b", "inception4c", "inception4d", "inception4e", None,
          "inception5a", "inception5b")


def cast(sd, dtype, device=None):
    return {k: (v.to(dtype=dtype, device=device) if v.is_floating_point() else v) for k, v in sd.items()}


def basic_conv(sd, prefix, x, stride=1, pad=0):
    """BasicConv2d: Conv2d(bias=False) -> BatchNorm2d(eps=0.001), running statistics -> ReLU"""
    x = F.conv2d(x, sd[prefix + ".conv.weight"], None, stride, pad)
    x = F.batch_norm(x, sd[prefix + ".bn.running_mean"], sd[prefix + ".bn.running_var"], sd[prefix + ".bn.weight"],
                     sd[prefix + ".bn.bias"], training=False, eps=0.001)
    return F.relu(x)


def inception(sd, name, x):
    b1 = basic_conv(sd, name + ".branch1", x)
    b2 = basic_conv(sd, name + ".branch2.1", basic_conv(sd, name + ".branch2.0", x), pad=1)
    b3 = basic_conv(sd, name + ".branch3.1", basic_conv(sd, name + ".branch3.0", x), pad=1)       # 3x3: torchvision's deviation
    b4 = basic_conv(sd, name + ".branch4.1", F.max_pool2d(x, 3, 1, 1, ceil_mode=True))
    return torch.cat([b1, b2, b3, b4], 1)


def forward(sd, x):
    """x: [N, 3, H, W], normalised; sd in x's dtype -> [N, 1024]"""
    x = basic_conv(sd, "conv1", x, 2, 3)
    x = F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    x = basic_conv(sd, "conv2", x)
    x = basic_conv(sd, "conv3", x, 1, 1)
    x = F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    pools = iter(((3, 2), (2, 2)))
    for name in BLOCKS:
        if name is None:
            k, s = next(pools)
            x = F.max_pool2d(x, k, s, 0, ceil_mode=True)
        else:
            x = inception(sd, name, x)
    return F.adaptive_avg_pool2d(x, (1, 1)).flatten(1)


def normalise(frames, dtype):
    """[N, H, W, 3] uint8 -> [N, 3, H, W]: ToTensor (x / 255) then Normalize(mean, std), in ``dtype``"""
    x = frames.permute(0, 3, 1, 2).to(dtype) / 255
    mean = torch.tensor(MEAN, dtype=dtype, device=frames.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype, device=frames.device).view(1, 3, 1, 1)
    return (x - mean) / std


def layer_sizes(h, w):
    """[(name, channels, h, w)] after every layer of the trunk, by torch's own layers on a one-channel tensor"""
    x = torch.zeros(1, 1, h, w)
    one = torch.zeros(1, 1, 1, 1)
    out = []
    x = F.conv2d(x, torch.zeros(1, 1, 7, 7), None, 2, 3); out.append(("conv1", 64, x.shape[2], x.shape[3]))
    x = F.max_pool2d(x, 3, 2, 0, ceil_mode=True); out.append(("maxpool1", 64, x.shape[2], x.shape[3]))
    x = F.conv2d(x, one); out.append(("conv2", 64, x.shape[2], x.shape[3]))
    x = F.conv2d(x, torch.zeros(1, 1, 3, 3), None, 1, 1); out.append(("conv3", 192, x.shape[2], x.shape[3]))
    x = F.max_pool2d(x, 3, 2, 0, ceil_mode=True); out.append(("maxpool2", 192, x.shape[2], x.shape[3]))
    widths = {"inception3a": 256, "inception3b": 480, "inception4a": 512, "inception4b": 512, "inception4c": 512,
              "inception4d": 528, "inception4e": 832, "inception5a": 832, "inception5b": 1024}
    pools = iter((("maxpool3", 3, 2), ("maxpool4", 2, 2)))
    c = 192
    for name in BLOCKS:
        if name is None:
            pname, k, s = next(pools)
            x = F.max_pool2d(x, k, s, 0, ceil_mode=True); out.append((pname, c, x.shape[2], x.shape[3]))
        else:
            y = F.max_pool2d(x, 3, 1, 1, ceil_mode=True)
            assert y.shape == x.shape
            c = widths[name]
            out.append((name, c, x.shape[2], x.shape[3]))
    return out
