"""What the pretraining-head tests share (test_pretrain.py, test_hip_pretrain_packed.py, test_hip_pretrain_head_edges.py): the
reference's formulas restated in float64 torch for the padded and for the packed head, and the fixture that pins the tiled GEMMs."""
import pytest
import torch


def head_reference(hidden, logits, vid, mask, W, b, temp, pen):
    """The reference's formulas (simnet_pretrain.py:35-98) restated op for op in float64 torch, [T,T] matrix included."""
    import torch.nn.functional as F
    feats = F.linear(hidden, W, b)
    x = feats * (mask == False).unsqueeze(2) if mask is not None else feats      # noqa: E712
    x = x / (x.norm(dim=2, keepdim=True) + 1e-9)
    T = x.shape[1]
    sim = torch.matmul(x, x.transpose(1, 2)) * (torch.eye(T, dtype=x.dtype) == 0).to(x.dtype).unsqueeze(0)
    repel = sim.mean(dim=1).mean()
    sc = logits
    if mask is not None:
        sc = sc.masked_fill(mask.unsqueeze(2), float("-inf"))
    mix = F.softmax(sc / temp, dim=1)
    if pen == "entropy":
        e = (mix + 1e-9) * torch.log(mix + 1e-9)
        if mask is not None:
            e = e.masked_fill(mask.unsqueeze(2), 0.)
        center = e.mean(dim=1).mean()
    else:
        center = torch.norm(mix, dim=1).mean()
    pooled = torch.matmul(mix.transpose(1, 2), feats).squeeze(1)
    loss = (-F.softmax(vid, dim=1) * torch.log(F.softmax(pooled, dim=1))).mean()
    return loss, center, repel


def head_reference_packed(hidden, logits, vid, lengths, W, b, temp, pen, ref_len):
    """The packed head's contract (include/vs_train.h) per video in float64 torch; the repelling term in the reference's
    own form, the [T,T] cosine matrix without its diagonal (simnet_pretrain.py:56-69), summed and divided by ref_len^2."""
    import torch.nn.functional as F
    feats = F.linear(hidden, W, b)
    main, center, repel = [], [], []
    row = 0
    for i, T in enumerate(lengths):
        f, s = feats[row:row + T], logits[row:row + T].reshape(T)
        row += T
        x = f / (f.norm(dim=1, keepdim=True) + 1e-9)
        sim = (x @ x.t()) * (torch.eye(T, dtype=x.dtype) == 0).to(x.dtype)
        repel.append(sim.sum() / float(ref_len * ref_len))
        w = F.softmax(s / temp, dim=0)
        if pen == "entropy":
            center.append(((w + 1e-9) * torch.log(w + 1e-9)).sum() / float(ref_len))
        else:
            center.append(torch.norm(w))
        pooled = (w.unsqueeze(0) @ f).squeeze(0)
        main.append((-F.softmax(vid[i], dim=0) * torch.log(F.softmax(pooled, dim=0))).mean())
    return torch.stack(main).mean(), torch.stack(center).mean(), torch.stack(repel).mean()


@pytest.fixture
def tiled_gemms(vsa):
    """VS_SKINNY_ROWS=0 pins the LDS-tiled GEMMs (video_transform's forward, dgrad and wgrad) that batches above the
    skinny threshold take; these small batches get the latency kernels by default."""
    vsa._lib.set_option("VS_SKINNY_ROWS", 0)
    yield
    vsa._lib.set_option("VS_SKINNY_ROWS", -1)
