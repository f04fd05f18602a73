"""The exact-fp32 layer tail as ONE kernel against the stand-alone kernels, bit for bit.

gemm_ln_rows_tail_qkv / gemm_ln_rows_tail_score run out-projection + LayerNorm1, fc1, fc2 + LayerNorm2 and the next
layer's QKV (or the score head) in one launch per layer: h1 stays in the accumulators and is never stored, and a block
reads back the hidden rows it has just written.  They promise the bits of the four stand-alone kernels, which VS_EXACT_UNFUSED=1 brings back:
every case runs both ways and asserts torch.equal on the logits (or sigmoid scores) and on the hidden state.
VS_SKINNY_ROWS=0 sends small batches to the tiled kernels and VS_LAYER_TAIL_MIN_ROWS=0 forces the one-launch kernel, so the
shapes are the smallest at which it can go wrong: tile edges, where fc1's dropped stores past M meet staged hidden rows that
were never written.  Synthetic weights (synth.make_state_dict), d_model 256.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture
def tail(vsa):
    vsa._lib.set_option("VS_SKINNY_ROWS", 0)
    vsa._lib.set_option("VS_LAYER_TAIL_MIN_ROWS", 0)
    yield
    vsa._lib.set_option("VS_SKINNY_ROWS", -1)
    vsa._lib.set_option("VS_LAYER_TAIL_MIN_ROWS", -1)
    vsa._lib.set_option("VS_EXACT_UNFUSED", -1)


def _model(vsa, H, L, seed, use_cls=False):
    sd = vsa.synth.make_state_dict(256, L, seed, use_cls=use_cls)
    m = vsa.SimNet(num_heads=H, d_model=256, num_layers=L, sparsity=0.0, dropout=0.3, use_cls=use_cls)
    m.load_state_dict(sd, strict=True)
    return m.to(_dev()).eval()


def _run(vsa, run, unfused):
    vsa._lib.set_option("VS_EXACT_UNFUSED", unfused)
    try:
        with torch.no_grad():
            out = [o.clone() for o in run()]
        torch.cuda.synchronize()
    finally:
        vsa._lib.set_option("VS_EXACT_UNFUSED", -1)
    return out


def _both_ways(vsa, run):
    """run() with the one-launch layer tail and with the stand-alone kernels; the former's result after the equality checks."""
    fused, alone = _run(vsa, run, 0), _run(vsa, run, 1)
    for a, b in zip(fused, alone):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), "layer tail and stand-alone kernels differ: max |diff| %.3e" % (a - b).abs().max().item()
    return fused


def _counts(vsa, m, x):
    lib = vsa._lib.load()
    with torch.no_grad():
        m(x)                                  # weights packed, workspace allocated
        torch.cuda.synchronize()
        vsa._lib.check(lib.vs_profile_enable(1))
        m(x)
        torch.cuda.synchronize()
        counts = {k: n for k, (_ms, n) in vsa._lib.profile_collect().items()}
        vsa._lib.check(lib.vs_profile_enable(0))
    return counts


@pytest.mark.parametrize("B,T", [(1, 1), (1, 127), (1, 129), (3, 100), (2, 128)])
def test_layer_tail_equals_the_stand_alone_kernels_at_tile_edges(vsa, tail, B, T):
    m = _model(vsa, 4, 4, 51)
    x = vsa.synth.make_features(B, T, 52 + T, "randn").to(_dev())
    _both_ways(vsa, lambda: m(x))


@pytest.mark.parametrize("L", [1, 2])
def test_one_layer_is_the_score_form_alone_and_two_layers_have_both(vsa, tail, L):
    m = _model(vsa, 4, L, 53)
    x = vsa.synth.make_features(2, 129, 54, "randn").to(_dev())
    _both_ways(vsa, lambda: m(x))


@pytest.mark.parametrize("H", [8, 4, 2])
def test_head_dims_32_64_128(vsa, tail, H):
    m = _model(vsa, H, 2, 55)
    x = vsa.synth.make_features(2, 130, 56 + H, "randn", lengths=[130, 77])
    mask = vsa.synth.padding_mask(x).to(_dev())
    xd = x.to(_dev())
    _both_ways(vsa, lambda: m(xd, mask))


def test_ragged_padded_batch_with_its_key_mask(vsa, tail):
    m = _model(vsa, 4, 4, 57)
    x = vsa.synth.make_features(3, 150, 58, "randn", lengths=[150, 129, 40])
    mask = vsa.synth.padding_mask(x).to(_dev())
    xd = x.to(_dev())
    _both_ways(vsa, lambda: m(xd, mask))


def test_class_token_forward(vsa, tail):
    m = _model(vsa, 4, 2, 59, use_cls=True)
    x = vsa.synth.make_features(2, 128, 60, "randn").to(_dev())
    logits, hidden = _both_ways(vsa, lambda: m(x))
    assert logits.shape == (2, 129, 1) and hidden.shape == (2, 129, 256)


def test_packed_batch_equals_scoring_each_video_alone(vsa, tail):
    m = _model(vsa, 4, 2, 61)
    lengths = [5, 130, 64]
    vids = [vsa.synth.make_features(1, t, 62 + i, "randn")[0] for i, t in enumerate(lengths)]
    x = torch.cat(vids, dim=0).to(_dev())
    logits, hidden = _both_ways(vsa, lambda: m.forward_packed(x, lengths))
    row = 0
    with torch.no_grad():
        for v, t in zip(vids, lengths):
            l1, h1 = m(v[None].to(_dev()))
            assert torch.equal(logits[row:row + t], l1[0]) and torch.equal(hidden[row:row + t], h1[0]), t
            row += t


def test_sigmoid_scores(vsa, tail):
    m = _model(vsa, 4, 2, 63)
    x = vsa.synth.make_features(2, 130, 64, "randn").to(_dev())
    (s,) = _both_ways(vsa, lambda: (m.score(x),))
    assert s.shape == (2, 130) and bool(((s > 0) & (s < 1)).all())


def test_one_launch_per_layer_with_the_threshold_at_zero_and_the_pair_above_it(vsa, tail):
    L = 3
    m = _model(vsa, 4, L, 65)
    x = vsa.synth.make_features(2, 100, 66, "randn").to(_dev())
    one = _counts(vsa, m, x)
    assert one["fc1_relu"] == 0 and one["outproj_ln"] == 0 and one["fc2_ln_score"] == L and one["qkv_proj"] == 1, one
    assert one["attention"] == L
    vsa._lib.set_option("VS_LAYER_TAIL_MIN_ROWS", 201)       # above M = 200: the two layer kernels of round 7
    pair = _counts(vsa, m, x)
    assert pair["fc1_relu"] == L and pair["outproj_ln"] == 0 and pair["fc2_ln_score"] == L and pair["qkv_proj"] == 1, pair


def test_twenty_runs_of_an_edge_case_give_identical_bits(vsa, tail):
    """A block reads hidden rows that other waves of it stored: a missing wait or barrier shows as run-to-run differences."""
    m = _model(vsa, 4, 4, 67)
    x = vsa.synth.make_features(3, 100, 68, "randn").to(_dev())
    first = _both_ways(vsa, lambda: m(x))
    for i in range(19):
        again = _run(vsa, lambda: m(x), 0)
        for a, b in zip(first, again):
            assert torch.equal(a, b), "run %d differs from run 0: max |diff| %.3e" % (i + 1, (a - b).abs().max().item())
