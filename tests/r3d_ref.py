"""The oracle of the R3D-18 video-level feature: our own restatement of torchvision's ``r3d_18`` up to and including ``avgpool``
(the reference's ``models.R3D18``), then ``flatten(1)``, in plain torch functions on torchvision's key names, in whatever dtype the
input has - float64 as the truth, float32 on the CPU as the yardstick for what fp32 arithmetic itself costs.  Written from the
architecture (stem 3x7x7 / (1,2,2); four layers of two BasicBlocks, planes 64 / 128 / 256 / 512, first-block stride 1 / 2 / 2 / 2
in all three dimensions; 1x1x1 stride-2 downsample on the identity of layer2..4's first block; the mean).  BatchNorm3d in eval
mode (running statistics), eps 1e-5.  F.conv3d, F.batch_norm, F.relu and the mean are the only operators."""
import torch
import torch.nn.functional as F

MEAN, STD = (0.43216, 0.394666, 0.37645), (0.22803, 0.22145, 0.216989)
EPS = 1e-5


def cast(sd, dtype, device=None):
    return {k: (v.to(dtype=dtype, device=device) if v.is_floating_point() else v) for k, v in sd.items()}


def conv_bn(sd, prefix, x, stride, pad):
    """``prefix.0`` Conv3d(bias=False) -> ``prefix.1`` BatchNorm3d, running statistics"""
    x = F.conv3d(x, sd[prefix + ".0.weight"], None, stride, pad)
    return F.batch_norm(x, sd[prefix + ".1.running_mean"], sd[prefix + ".1.running_var"], sd[prefix + ".1.weight"], sd[prefix + ".1.bias"],
                        training=False, eps=EPS)


def basic_block(sd, prefix, x, stride):
    out = F.relu(conv_bn(sd, prefix + ".conv1", x, stride, 1))
    out = conv_bn(sd, prefix + ".conv2", out, 1, 1)
    identity = conv_bn(sd, prefix + ".downsample", x, 2, 0) if prefix + ".downsample.0.weight" in sd else x
    return F.relu(out + identity)


def forward(sd, x):
    """x: [N, 3, T, H, W], normalised; sd in x's dtype -> [N, 512]"""
    x = F.relu(conv_bn(sd, "stem", x, (1, 2, 2), (1, 3, 3)))
    for layer in (1, 2, 3, 4):
        x = basic_block(sd, "layer%d.0" % layer, x, 1 if layer == 1 else 2)
        x = basic_block(sd, "layer%d.1" % layer, x, 1)
    return x.mean(dim=(2, 3, 4))


def normalise(frames, dtype):
    """[N, T, H, W, 3] uint8 -> [N, 3, T, H, W]: ToTensor (x / 255) then Normalize(mean, std) frame by frame, stacked and
    permuted as the reference does, in ``dtype``"""
    x = frames.permute(0, 4, 1, 2, 3).to(dtype) / 255
    mean = torch.tensor(MEAN, dtype=dtype, device=frames.device).view(1, 3, 1, 1, 1)
    std = torch.tensor(STD, dtype=dtype, device=frames.device).view(1, 3, 1, 1, 1)
    return (x - mean) / std
