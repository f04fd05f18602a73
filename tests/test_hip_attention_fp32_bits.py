"""Bit identity of the exact-fp32 attention (attn_fwd_pipe) across the rescheduling of its tile loop (DESIGN.md section 5,
round 8): the row bias as the C operand of a block's first S' MFMA, the block maximum as a tree, two tiles per loop iteration.

tests/golden/attention_fp32_bits.json holds the sha256 of every case's output bytes, recorded by
tests/golden/make_golden_attention_bits.py on the commit before the change, and that build's own distance from the float64
reference.  Each case must reproduce its hash and stay within its limit of the reference: 2e-5 for the random-input cases
(test_hip_parity.py::test_attention_kernel), 5e-5 for the two spiked ones (test_attention_online_softmax_rescale_branch) - the
recording build measured 4.2e-5 on both, inside it.  Two cases are the inputs on which a first version of the change returned
wrong results in the masked head-dim-32 kernels.  The cases are listed, with what each is for, in tests/attention_bits_cases.py.
"""
import json
import os

import pytest
import torch

import attention_bits_cases as abc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_fp32_bits.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", [c[0] for c in abc.DIRECT] + abc.SPIKED)
def test_attention_bits(vsa, golden, name):
    spiked = name in abc.SPIKED
    q, k, v, mask, scale = abc.spiked_inputs(name) if spiked else abc.direct_inputs(vsa.synth, name)
    want = golden["direct"][name]
    assert want["limit"] == (abc.LIMIT_RESCALE if spiked else abc.LIMIT_RANDOM) and want["recorded_err"] < want["limit"]
    out = abc.run_direct(vsa, q, k, v, mask, scale, _dev())
    err = (out.double() - abc.attn_ref(q, k, v, mask, scale)).abs().max().item()
    print("%s: max |out - float64| %.3e (recorded %.3e, limit %.1e)" % (name, err, want["recorded_err"], want["limit"]))
    assert err < want["limit"]
    assert abc.sha(out) == want["sha256"]
    assert abc.sha(abc.run_direct(vsa, q, k, v, mask, scale, _dev())) == want["sha256"]        # the same call again


def test_spiked_cases_raise_the_maximum(vsa):
    """The spiked inputs do what they are for: key 300 lifts the row maximum (log2 units) by more than 2^8 over everything
    before it, in every head, for some query of every wave's 32 rows; in spike_twice key 270 lifts it by more than 2^8 first."""
    log2e = 1.4426950408889634
    for name in abc.SPIKED:
        q, k, _, _, scale = abc.spiked_inputs(name)
        s = torch.matmul(q.double(), k.double().transpose(2, 3)) * scale * log2e        # [B, H, T, T]
        for key, before in ((300, 288), (270, 256)) if name == "spike_twice" else ((300, 288),):
            jump = s[..., key] - s[..., :before].max(dim=3).values                       # [B, H, T]
            per_wave = jump.reshape(jump.shape[0], jump.shape[1], -1, 32).max(dim=3).values
            assert (per_wave > 8.0).all(), (name, key, per_wave.min().item())


def test_packed_ragged_bits(vsa, golden):
    """One packed call over lengths that end inside, on and just past a tile and a block: the hashes of the recording build,
    scores bit-equal to the padded batch's and to each video scored alone, and the same bytes when called again."""
    m = abc.packed_model(vsa, _dev())
    vids = abc.packed_videos(vsa.synth)
    lengths = abc.PACKED_LENGTHS
    x = torch.cat(vids).to(_dev())
    want = golden["packed"]
    assert want["scores_equal_padded_batch"] and want["scores_equal_each_alone"]
    with torch.no_grad():
        logits, hidden = m.forward_packed(x, lengths)
        sc = m.score_packed(x, lengths)
        xp = torch.full((len(vids), max(lengths), vids[0].shape[1]), vsa.synth.PAD_VALUE)
        for i, vv in enumerate(vids):
            xp[i, :vv.shape[0]] = vv
        pm = vsa.synth.padding_mask(xp)
        padded = m.score(xp.to(_dev()), pm.to(_dev())).cpu()
        alone = torch.cat([m.score(vv[None].to(_dev()))[0] for vv in vids]).cpu()
        again = m.score_packed(x, lengths)
    assert abc.sha(logits) == want["logits"] and abc.sha(hidden) == want["hidden"] and abc.sha(sc) == want["scores"]
    assert torch.equal(padded[~pm], sc.cpu())
    assert torch.equal(alone, sc.cpu())
    assert torch.equal(again, sc)
