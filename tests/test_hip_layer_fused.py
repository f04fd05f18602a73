"""Exact-fp32 layer kernels of d_model 256 against the kernels they replace, bit for bit.

layer_outproj_ln_fc1 (out-projection + residual + LayerNorm1, then fc1 + ReLU from the registers that hold the normalised
rows) and layer_fc2_ln_qkv (fc2 + residual + LayerNorm2, then the next layer's QKV the same way) promise the bits of the
four stand-alone kernels: VS_EXACT_UNFUSED=1 brings those back, and every case here runs both ways and asserts torch.equal
on the logits (or sigmoid scores) and on the hidden state.  VS_SKINNY_ROWS=0 sends small batches to the tiled and fused
kernels, so the shapes can be the smallest at which tiling can go wrong: one row, one row short of and past a 128-row tile,
a tile edge inside a video, two exact tiles.  Synthetic weights (synth.make_state_dict), d_model 256.
"""
import pytest
import torch

import tolerances as tol
from oracle.simnet_oracle import oracle_forward

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture
def tiled(vsa):
    vsa._lib.set_option("VS_SKINNY_ROWS", 0)
    yield
    vsa._lib.set_option("VS_SKINNY_ROWS", -1)
    vsa._lib.set_option("VS_EXACT_UNFUSED", -1)


def _model(vsa, H, L, seed, use_cls=False):
    sd = vsa.synth.make_state_dict(256, L, seed, use_cls=use_cls)
    m = vsa.SimNet(num_heads=H, d_model=256, num_layers=L, sparsity=0.0, dropout=0.3, use_cls=use_cls)
    m.load_state_dict(sd, strict=True)
    return sd, m.to(_dev()).eval()


def _both_ways(vsa, run):
    """run() with the fused kernels (the default) and with the stand-alone ones; the fused result after the equality checks."""
    outs = []
    for unfused in (0, 1):
        vsa._lib.set_option("VS_EXACT_UNFUSED", unfused)
        with torch.no_grad():
            outs.append([o.clone() for o in run()])
        torch.cuda.synchronize()
    vsa._lib.set_option("VS_EXACT_UNFUSED", -1)
    for a, b in zip(*outs):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), "fused and stand-alone kernels differ: max |diff| %.3e" % (a - b).abs().max().item()
    return outs[0]


@pytest.mark.parametrize("B,T", [(1, 1), (1, 127), (1, 129), (3, 100), (2, 128)])
def test_fused_layers_equal_the_stand_alone_kernels_at_tile_edges(vsa, tiled, B, T):
    _, m = _model(vsa, 4, 4, 31)
    x = vsa.synth.make_features(B, T, 32 + T, "randn").to(_dev())
    _both_ways(vsa, lambda: m(x))


def test_more_row_tiles_than_resident_blocks(vsa):
    """B=65, T=1024: 520 row tiles on a grid of two blocks per CU (512 on the MI355X), so some blocks walk a second tile
    while their CU's other block is still storing its first one - the co-residence under which a chunk's last read-back
    through the transposition corner was once overtaken by the next chunk block's writes."""
    _, m = _model(vsa, 4, 2, 47)
    x = torch.randn(65, 1024, 1024, device=_dev(), generator=torch.Generator(device=_dev()).manual_seed(48))
    _both_ways(vsa, lambda: m(x))


def test_fused_layers_launch_in_place_of_the_stand_alone_kernels(vsa, tiled):
    """The default path really runs the two layer kernels: no out-projection launch of its own, one QKV launch (layer 0's)."""
    lib = vsa._lib.load()
    L = 3
    _, m = _model(vsa, 4, L, 33)
    x = vsa.synth.make_features(2, 100, 34, "randn").to(_dev())
    counts = {}
    for unfused in (0, 1):
        vsa._lib.set_option("VS_EXACT_UNFUSED", unfused)
        with torch.no_grad():
            m(x)                                  # weights packed, workspace allocated
            torch.cuda.synchronize()
            vsa._lib.check(lib.vs_profile_enable(1))
            m(x)
            torch.cuda.synchronize()
            counts[unfused] = {k: n for k, (_ms, n) in vsa._lib.profile_collect().items()}
            vsa._lib.check(lib.vs_profile_enable(0))
    assert counts[1]["outproj_ln"] == L and counts[1]["qkv_proj"] == L and counts[1]["fc1_relu"] == L, counts[1]
    assert counts[0]["outproj_ln"] == 0 and counts[0]["qkv_proj"] == 1 and counts[0]["fc1_relu"] == L, counts[0]
    assert counts[0]["fc2_ln_score"] == L and counts[0]["attention"] == L


def test_key_padding_mask_and_the_oracle(vsa, tiled):
    """A ragged padded batch with its key-padding mask; this case is also held to the CPU oracle at the 1e-4 bar."""
    sd, m = _model(vsa, 4, 4, 35)
    x = vsa.synth.make_features(3, 150, 36, "randn", lengths=[150, 129, 40])
    mask = vsa.synth.padding_mask(x)
    xd, md = x.to(_dev()), mask.to(_dev())
    logits, hidden = _both_ways(vsa, lambda: m(xd, md))
    with torch.no_grad():
        rl, rh = oracle_forward(sd, x, mask, 4)
    valid = ~mask
    e1 = (logits.cpu() - rl)[valid].abs().max().item()
    e2 = (hidden.cpu() - rh)[valid].abs().max().item()
    print("fused layers vs oracle: max |logit err| %.3e  max |hidden err| %.3e" % (e1, e2))
    assert e1 < tol.FP32_TOL and e2 < tol.FP32_TOL


def test_sigmoid_scores(vsa, tiled):
    _, m = _model(vsa, 4, 2, 37)
    x = vsa.synth.make_features(2, 130, 38, "randn").to(_dev())
    (s,) = _both_ways(vsa, lambda: (m.score(x),))
    assert s.shape == (2, 130) and bool(((s > 0) & (s < 1)).all())


@pytest.mark.parametrize("L", [1, 2])
def test_one_layer_has_no_fused_qkv_and_two_layers_have_both_forms(vsa, tiled, L):
    """L = 1: the only fc2 kernel is the last layer's (LayerNorm2 + score head, no QKV); L = 2: one of each."""
    _, m = _model(vsa, 4, L, 39)
    x = vsa.synth.make_features(2, 129, 40, "randn").to(_dev())
    _both_ways(vsa, lambda: m(x))


@pytest.mark.parametrize("H", [8, 4, 2])
def test_head_dims_32_64_128(vsa, tiled, H):
    """The QKV tail scatters 32-column blocks into head-major planes: the head dim decides where each block goes."""
    _, m = _model(vsa, H, 2, 41)
    x = vsa.synth.make_features(2, 130, 42 + H, "randn", lengths=[130, 77])
    mask = vsa.synth.padding_mask(x).to(_dev())
    xd = x.to(_dev())
    _both_ways(vsa, lambda: m(xd, mask))


def test_class_token_forward(vsa, tiled):
    """use_cls: T + 1 rows per video, so the rows of a video no longer start at a multiple of T in the QKV scatter."""
    _, m = _model(vsa, 4, 2, 43, use_cls=True)
    x = vsa.synth.make_features(2, 128, 44, "randn").to(_dev())
    logits, hidden = _both_ways(vsa, lambda: m(x))
    assert logits.shape == (2, 129, 1) and hidden.shape == (2, 129, 256)


def test_packed_batch_equals_scoring_each_video_padded(vsa, tiled):
    """A packed ragged batch (the QKV tail then runs as B = 1, T = all rows): equal both ways, and every video's rows equal
    the same video scored through the padded entry point, bit for bit, as the packed tests of test_hip_parity.py require."""
    _, m = _model(vsa, 4, 2, 45)
    lengths = [5, 130, 64]
    vids = [vsa.synth.make_features(1, t, 46 + i, "randn")[0] for i, t in enumerate(lengths)]
    x = torch.cat(vids, dim=0).to(_dev())
    logits, hidden = _both_ways(vsa, lambda: m.forward_packed(x, lengths))
    row = 0
    with torch.no_grad():
        for v, t in zip(vids, lengths):
            l1, h1 = m(v[None].to(_dev()))
            assert torch.equal(logits[row:row + t], l1[0]) and torch.equal(hidden[row:row + t], h1[0]), t
            row += t
