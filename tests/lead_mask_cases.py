"""Key masks whose LEADING keys are dead, shared by tests/test_lead_mask_cases_host.py (properties of the masks, fp32 head-room
of the bounds) and tests/test_hip_attention_lead_mask.py (every attention kernel on them).

Every attention kernel guards the state "this row has seen no live key yet" (running maximum -inf) by hand; a key mask reaches
that state only when it kills key 0, which synth.random_mask and every other mask of the suite avoid.  Here the batch dimension
carries the position of the first live key: video b of a T-frame case has keys < first_live(T)[b] dead.

Lengths, and the stride each is there for:
  65   4-wave scoring blocks, two 64-key tiles, the last tile holds one key; three 32-key training tiles
  200  8-wave blocks and the one-wave-per-SIMD route, four tiles with a ragged fourth; two 128-row owner tiles
  320  4-wave blocks, three query tiles, T % 64 == 0
  449  the wide route again: eight tiles (more than the ring of three), key 448 alone in the last tile
Positions: 1; 31 / 32 / 33 (the 32-key blocks of the scoring kernels, the 32-row streamed tiles of the exact training kernels);
one key either side of every multiple of 64 up to 448 (64-key tiles, the 64-row tiles of the 16-bit training kernels, the
split-key kernel's wave w taking tiles w, w + 8, ...; the multiples of 128 are the two-tiles-per-iteration loop of 8-wave blocks
and the 128-row owner tiles; from 192 on the first live tile lies beyond the ring of three); and T - 1, where the only live key
is the last one - at T = 65 and 449 alone in a ragged last tile, the peeled tile's softmax_only.
"""
import functools

import numpy as np
import torch

LENGTHS = (65, 200, 320, 449)
POSITIONS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 447, 448)
FAMILIES = ("lead", "mixed")
HOLE_P = 0.3


def first_live(T):
    """the first-live positions of a T-frame case, ascending: video b uses first_live(T)[b]; the last one is T - 1"""
    return tuple(sorted({f for f in POSITIONS if f < T} | {T - 1}))


@functools.lru_cache(maxsize=None)
def _mask_np(T, family):
    F = first_live(T)
    m = np.zeros((len(F), T), dtype=bool)
    rng = np.random.Generator(np.random.PCG64(7000 + T))
    holes = rng.random(size=m.shape) < HOLE_P
    for b, f in enumerate(F):
        m[b, :f] = True
        if family == "mixed":
            m[b, f + 1:] = holes[b, f + 1:]
            tail = b % 7 + 1
            if b % 2 == 1 and T - tail > f:                # every second video: a dead tail that leaves key f alive
                m[b, T - tail:] = True
    assert family in FAMILIES and not m.all(axis=1).any()
    return m


def mask(T, family):
    """bool [B, T], True = dead key; B = len(first_live(T)).
    lead: keys < f dead, the rest live.  mixed: keys < f dead, key f live, every later key dead with probability 0.3, and in every
    second video the last b % 7 + 1 keys dead as well (unless that would kill key f)."""
    return torch.from_numpy(_mask_np(T, family).copy())


def only_last_live(T):
    """index of the video whose first live key is T - 1 (in the lead family: its only live key)"""
    return len(first_live(T)) - 1


def qkv(B, H, T, dh, seed):
    """(q, k, v fp32 [B, H, T, dh], scale): unit-gain randn.  At gain 2 a plain fp32 torch attention on these masks is already
    1.4e-5 from float64 at head dim 128, too close to the exact kernels' 2e-5; at unit gain it stays below 1e-6."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, T, dh, generator=g) for _ in range(3))
    return q, k, v, (H * dh) ** -0.5


@functools.lru_cache(maxsize=None)
def case_inputs(T, dh, H=2):
    """the inputs every test of a (T, head dim) uses: q, k, v, scale and the upstream gradient dO [B, T, H * dh]; drawn once,
    shared, never written to.
    dO has gain 1/8: in the one-hot video dv[T - 1] is the sum of all T rows of dO, about 3 sqrt(T) at unit gain, and
    TRAIN_GRAD_ATOL (1e-4 absolute) on an entry of 60 would ask 1.7e-6 relative of fp32 sums of 320 terms."""
    B = len(first_live(T))
    q, k, v, scale = qkv(B, H, T, dh, 1000 * dh + T)
    dO = torch.randn(B, T, H * dh, generator=torch.Generator().manual_seed(9000 + T + dh)) * 0.125
    return q, k, v, scale, dO


def attention(q, k, v, key_mask, scale, keep=None, p=0.0):
    """softmax(q k^T scale + key mask) with optional dropout keep bytes [B, H, T, T], times v, in the dtype of q (float64: the
    checker; float32: the plain restatement whose own error the host test holds 4x inside every bound).
    Returns (out [B, T, H * dh], lse2 [B, H, T], probabilities before dropout [B, H, T, T])."""
    B, H, T, dh = q.shape
    s = torch.matmul(q, k.transpose(2, 3)) * scale
    s = s.masked_fill(key_mask.view(B, 1, 1, T), float("-inf"))
    lse2 = torch.logsumexp(s, dim=3) / float(np.log(2.0))
    P = torch.softmax(s, dim=3)
    w = P if keep is None or p <= 0.0 else P * keep.to(P.dtype) / (1.0 - p)
    return torch.matmul(w, v).permute(0, 2, 1, 3).reshape(B, T, H * dh), lse2, P


def attention_grads(q, k, v, key_mask, scale, dO, dtype, keep=None, p=0.0):
    """(out, lse2, P, dq, dk, dv) by torch autograd in `dtype`; the gradients token-major [B, T, H * dh] like the kernels' dqkv"""
    B, H, T, dh = q.shape
    qq, kk, vv = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    out, lse2, P = attention(qq, kk, vv, key_mask, scale, keep, p)
    out.backward(dO.to(dtype))
    tok = lambda g: g.permute(0, 2, 1, 3).reshape(B, T, H * dh)       # noqa: E731
    return out.detach(), lse2.detach(), P.detach(), tok(qq.grad), tok(kk.grad), tok(vv.grad)


_REF = {}


def reference64(T, dh, family):
    """float64 (out, lse2, P, dq, dk, dv) of a case without dropout: computed once, shared, never written to"""
    key = (T, dh, family)
    if key not in _REF:
        q, k, v, scale, dO = case_inputs(T, dh)
        _REF[key] = attention_grads(q, k, v, mask(T, family), scale, dO, torch.float64)
    return _REF[key]
