"""GPU: the weight image families that tests/test_hip_train.py::test_parameter_updates_reach_every_kernel_layout_copy never
reaches (the family table of vs_weights.cpp) - the row-major bf16 copies, read by the bf16-operand GEMM of
d_model > 256 and by the training path's A-stationary GEMM; the transposes and their fragment-major copies at a latency-sized
batch; the bf16 copy of W2^T.  Each case builds its families once, changes the parameters in place (a torch write, or a native
Adam step, which bumps the handle's version itself) and then asks for the SAME BITS as a freshly packed module with the same values:
a family that was not rebuilt, or rebuilt from the wrong place, cannot give them.  One video of 90 frames, 2 layers."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


def _fresh(vsa, state, d, heads):
    m = vsa.SimNet(num_heads=heads, d_model=d, num_layers=2, sparsity=0.0, dropout=0.0)
    m.load_state_dict(state)
    return m.to(_dev())


def _state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _step(m, x):
    """one training forward and backward: the scores and every gradient"""
    m.train()
    m.zero_grad(set_to_none=True)
    scores, _ = m(x)
    scores.square().mean().backward()
    return [scores.detach().clone()] + [p.grad.clone() for p in m.parameters()]


def _write_in_place(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for prm in m.parameters():
            prm.add_(0.01 * torch.randn(prm.shape, generator=g).to(prm.device))


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), "%s: tensor %d differs" % (what, i)


def test_bf16_scoring_on_the_bf16_operand_gemm_sees_parameter_writes(vsa):
    x = vsa.synth.make_features(1, 90, 3, "randn").to(_dev())
    try:
        vsa._lib.set_option("VS_LP_MIN_ROWS", 0)
        m = _fresh(vsa, vsa.synth.make_state_dict(512, 2, 19), 512, 8).eval().set_compute_dtype("bf16")
        with torch.no_grad():
            m(x)                                            # builds the row-major bf16 copies
            _write_in_place(m, 7)
            ref = _fresh(vsa, _state(m), 512, 8).eval().set_compute_dtype("bf16")
            _same(m(x), ref(x), "bf16 scoring, d_model 512")
    finally:
        vsa._lib.set_option("VS_LP_MIN_ROWS", -1)


def test_bf16_training_on_the_a_stationary_gemm_sees_parameter_writes(vsa):
    x = vsa.synth.make_features(1, 90, 4, "randn").to(_dev())
    try:
        vsa._lib.set_option("VS_TRAIN_LP_MIN_ROWS", 0)
        vsa._lib.set_option("VS_LP_MLP_UNFUSED", 2)
        m = _fresh(vsa, vsa.synth.make_state_dict(256, 2, 29), 256, 4).set_train_dtype("bf16")
        _step(m, x)                                         # builds the row-major copies, the transposes and the bf16 W2^T
        _write_in_place(m, 8)
        ref = _fresh(vsa, _state(m), 256, 4).set_train_dtype("bf16")
        _same(_step(m, x), _step(ref, x), "bf16 training step, d_model 256")
    finally:
        vsa._lib.set_option("VS_TRAIN_LP_MIN_ROWS", -1)
        vsa._lib.set_option("VS_LP_MLP_UNFUSED", -1)


def test_fp32_training_after_a_native_adam_step(vsa):
    x = vsa.synth.make_features(1, 90, 5, "randn").to(_dev())
    m = _fresh(vsa, vsa.synth.make_state_dict(256, 2, 39), 256, 4)
    opt = vsa.Adam(m.parameters(), lr=1e-3).attach(m)
    _step(m, x)                                             # builds the transposes and their fragment-major copies (90 rows)
    opt.step()                                              # writes the packed copy and bumps its version: no re-pack
    ref = _fresh(vsa, _state(m), 256, 4)
    _same(_step(m, x), _step(ref, x), "fp32 training step after a native Adam step")
