"""Test infrastructure (not product code): a plain-torch restatement of ``SimNet.forward`` in EVAL mode (reference
src/model/simnet.py:32-45, 105-114, 138-164, 180-183) for ONE video without padding, that also returns every layer's softmax
weights - the tensors the reference appends to ``attention_maps`` (:112-113, 155-158).  Run in float64 on the CPU it is the
yardstick of the packed attention maps: a packed batch is checked video by video against it."""
import torch
import torch.nn.functional as F


def forward_with_maps(params, x, num_heads):
    """params: dict name -> tensor (reference state_dict names, any float dtype); x [T, in_features] of the same dtype.
    Returns (logits [T, nc], hidden [T, d], maps: one [H, T, T] tensor per layer)."""
    T = x.shape[0]
    d = params["embedding_layer.feature_transform.weight"].shape[0]
    H, dh = num_heads, d // num_heads
    h = F.linear(x, params["embedding_layer.feature_transform.weight"], params["embedding_layer.feature_transform.bias"])
    pe = params.get("embedding_layer.positional_encoding.pos_embedding")
    if pe is not None:
        h = h + pe[0, :T].to(h.dtype)
    L = 0
    while "encoder.module_list.%d.sa.q.weight" % L in params:
        L += 1
    scale = d ** -0.5                                                                  # simnet.py:126
    maps = []
    for l in range(L):
        pre = "encoder.module_list.%d." % l
        lin = lambda t, n: F.linear(t, params[pre + n + ".weight"], params[pre + n + ".bias"])     # noqa: E731
        q = lin(h, "sa.q").view(T, H, dh).permute(1, 0, 2)
        k = lin(h, "sa.k").view(T, H, dh).permute(1, 0, 2)
        v = lin(h, "sa.v").view(T, H, dh).permute(1, 0, 2)
        w = F.softmax(torch.matmul(q, k.transpose(1, 2)) * scale, dim=2)
        maps.append(w)
        o = lin(torch.matmul(w, v).permute(1, 0, 2).contiguous().view(T, d), "sa.feature_projection")
        h = F.layer_norm(o + h, (d,), params[pre + "norm1.weight"], params[pre + "norm1.bias"], 1e-5)
        f = lin(F.relu(lin(h, "mlp.fc1")), "mlp.fc2")
        h = F.layer_norm(f + h, (d,), params[pre + "norm2.weight"], params[pre + "norm2.bias"], 1e-5)
    return F.linear(h, params["final_layer.weight"], params["final_layer.bias"]), h, maps


def float64_video(sd, x, num_heads):
    """``forward_with_maps`` in float64 on the CPU, as numpy: (logits, maps [L, H, T, T])"""
    with torch.no_grad():
        logits, _, maps = forward_with_maps({k: v.double().cpu() for k, v in sd.items()}, x.double().cpu(), num_heads)
    return logits.numpy(), torch.stack(maps).numpy()
