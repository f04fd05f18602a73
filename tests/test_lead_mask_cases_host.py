"""CPU: the masked-leading-key cases of tests/lead_mask_cases.py - the masks are what they claim to be, and the bounds the GPU
tests hold the exact fp32 kernels to leave room: a plain fp32 torch restatement of the same attention stays at least 4x inside
each of them against float64 (2e-5 on the output, TRAIN_GRAD_ATOL / TRAIN_GRAD_RTOL on dq / dk / dv, FP32_TOL on maps, received
and entropy).  If the 4x did not hold for a case, the remedy would be a lower gain for that case, never a wider bound."""
import numpy as np
import pytest
import torch

import attn_cases
import lead_mask_cases as lm
from tolerances import FP32_TOL, TRAIN_GRAD_ATOL, TRAIN_GRAD_RTOL

OUT_TOL = 2e-5              # tests/test_hip_parity.py: test_attention_kernel
HEADROOM = 4.0


def test_positions_are_the_listed_ones():
    assert lm.LENGTHS == (65, 200, 320, 449)
    assert lm.first_live(65) == (1, 31, 32, 33, 63, 64)
    assert lm.first_live(200) == (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 199)
    assert lm.first_live(320) == (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319)
    assert lm.first_live(449) == lm.POSITIONS and lm.POSITIONS[-1] == 448
    for T in lm.LENGTHS:
        assert lm.first_live(T)[lm.only_last_live(T)] == T - 1


@pytest.mark.parametrize("T", lm.LENGTHS)
def test_mask_families(T):
    F = lm.first_live(T)
    lead, mixed = lm.mask(T, "lead").numpy(), lm.mask(T, "mixed").numpy()
    assert lead.shape == mixed.shape == (len(F), T) and lead.dtype == mixed.dtype == np.bool_
    for b, f in enumerate(F):
        for m in (lead, mixed):
            assert m[b, :f].all() and not m[b, f], (b, f)                      # keys < f dead, key f live: a live key in every video
        assert not lead[b, f:].any()
    b = lm.only_last_live(T)
    assert (~lead[b]).sum() == 1 and not lead[b, T - 1]                          # the one-hot video
    assert np.array_equal(lm.mask(T, "mixed").numpy(), mixed)                   # seeded
    # mixed really has holes (dead keys between live ones) and tails (every second video, where key f survives it)
    later = np.concatenate([mixed[b, f + 1:] for b, f in enumerate(F)])
    assert 0.2 < later.mean() < 0.45, later.mean()
    holes = sum(int(mixed[b, f + 1:np.flatnonzero(~mixed[b])[-1]].sum()) for b, f in enumerate(F))
    assert holes > 0
    tails = [b for b, f in enumerate(F) if b % 2 == 1 and T - (b % 7 + 1) > f]
    assert tails and all(mixed[b, T - (b % 7 + 1):].all() for b in tails)
    assert any(not mixed[b, T - 1] for b in range(0, len(F), 2))                 # and some videos end on a live key


def _entropy(P):
    return -torch.where(P > 0, P * torch.log(P), torch.zeros_like(P)).sum(dim=3)


@pytest.mark.parametrize("dh", [32, 64, 128, 256])
@pytest.mark.parametrize("T", lm.LENGTHS)
def test_fp32_restatement_is_four_times_inside_every_exact_bound(T, dh):
    q, k, v, scale, dO = lm.case_inputs(T, dh)
    assert q.dtype == torch.float32 and abs(q.std().item() - 1.0) < 0.05         # unit gain
    for family in lm.FAMILIES:
        mask = lm.mask(T, family)
        o64, l64, P64, *g64 = lm.reference64(T, dh, family)
        o32, l32, P32, *g32 = lm.attention_grads(q, k, v, mask, scale, dO, torch.float32)
        assert all(torch.isfinite(t).all() for t in (o64, l64, o32, l32, *g64, *g32))
        valid = ~mask.numpy()
        rec64, ent64 = attn_cases.reductions64(P64.numpy(), valid)
        w = (~mask).float()[:, None, :, None]
        rec32 = (P32 * w).sum(dim=2) / (~mask).sum(dim=1).float()[:, None, None]
        vq = np.broadcast_to(valid[:, None, :], ent64.shape)
        e_out = (o32.double() - o64).abs().max().item()
        e_map = (P32.double() - P64).abs().max().item()
        e_rec = np.abs(rec32.double().numpy() - rec64).max()
        e_ent = np.abs(_entropy(P32).double().numpy() - ent64)[vq].max()
        e_g = [((a.double() - b).abs().max().item(), b.abs().max().item()) for a, b in zip(g32, g64)]
        print("T %3d dh %3d %-5s: out %.1e  map %.1e received %.1e entropy %.1e  dq %.1e/%.2f dk %.1e/%.2f dv %.1e/%.2f"
              % ((T, dh, family, e_out, e_map, e_rec, e_ent) + tuple(x for pair in e_g for x in pair)))
        assert HEADROOM * e_out <= OUT_TOL, e_out
        assert HEADROOM * max(e_map, e_rec, e_ent) <= FP32_TOL, (e_map, e_rec, e_ent)
        for (err, big), name in zip(e_g, ("dq", "dk", "dv")):
            assert HEADROOM * err <= TRAIN_GRAD_ATOL and HEADROOM * err <= TRAIN_GRAD_RTOL * big + 1e-6, (name, err, big)
        # what the exact assertions of the GPU tests rest on holds in the references themselves: dead keys get no gradient
        dead = mask[:, :, None].expand_as(g64[1])
        assert (g64[1][dead] == 0).all() and (g64[2][dead] == 0).all()
