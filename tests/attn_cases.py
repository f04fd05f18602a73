"""The attention-map golden cases and their recipe, shared by tests/golden/make_golden_attn.py (which runs the imported
reference on them) and the tests (which rebuild the same weights and inputs for the HIP path).

The seeded weights of ``synth.make_state_dict`` give near-uniform attention (every map within 1.4e-2 of 1/n, every row
entropy >= 0.995 log n): a kernel returning 1/n would nearly pass.  The cases therefore multiply the q and k projections
of every layer by a gain ``g``: at g = 4 the median row entropy is 0.6-0.9 log n with peaks up to 0.98, at g = 8 rows are
close to one-hot.  g = 16 is excluded: there the reference's own fp32 path is 3e-4 from its float64 run.
"""
import numpy as np
import torch

QK_SUFFIXES = ("sa.q.weight", "sa.q.bias", "sa.k.weight", "sa.k.bias")

# full: the fixture holds every map row (T <= 100); otherwise every `stride`-th query row, or none (summaries only)
CASES = [
    dict(name="attn_d256_h4_t96_randmask_g4", d=256, H=4, L=2, B=2, T=96, wseed=31, xseed=301, randmask=311, g=4, stride=1),
    dict(name="attn_d256_h8_t65_g8", d=256, H=8, L=2, B=1, T=65, wseed=32, xseed=302, g=8, stride=1),
    dict(name="attn_d256_h1_t150_pad_g8", d=256, H=1, L=2, B=2, T=150, wseed=33, xseed=303, lengths=[150, 101], g=8, stride=7),
    dict(name="attn_d1024_h8_t97_g4", d=1024, H=8, L=1, B=1, T=97, wseed=34, xseed=304, g=4, stride=1),
    dict(name="attn_d200_h5_t130_g4", d=200, H=5, L=2, B=2, T=130, wseed=35, xseed=305, g=4, stride=7),
    dict(name="attn_d256_h4_t320_pad_g1", d=256, H=4, L=4, B=2, T=320, wseed=36, xseed=306, lengths=[320, 211], g=1, stride=32),
    dict(name="attn_cls_d256_h4_t97_g4", d=256, H=4, L=2, B=2, T=97, wseed=37, xseed=307, g=4, stride=1, use_cls=True),
    dict(name="attn_d256_h4_t2000_g4", d=256, H=4, L=4, B=1, T=2000, wseed=38, xseed=308, g=4, stride=0),
]


def apply_gain(sd, g):
    """A copy of the state dict with every layer's q / k projection (weight and bias) multiplied by g."""
    return {k: (v * float(g) if k.endswith(QK_SUFFIXES) else v.clone()) for k, v in sd.items()}


def qk_checksum(sd):
    """float64 sum of |.| over the q / k projections: written into each fixture by the generator, recomputed by the tests"""
    return float(sum(v.double().abs().sum().item() for k, v in sd.items() if k.endswith(QK_SUFFIXES)))


def build(synth, c):
    """(state dict with the gain applied, x, mask or None) of a case"""
    sd = synth.make_state_dict(c["d"], c["L"], c["wseed"], use_cls=bool(c.get("use_cls")))
    if c.get("use_cls"):
        sd["embedding_layer.cls_token"] = sd["embedding_layer.cls_token"] * 0.5      # the seeded N(0,1) token, halved
    sd = apply_gain(sd, c["g"])
    x = synth.make_features(c["B"], c["T"], c["xseed"], "randn", c.get("lengths"))
    mask = None
    if c.get("lengths") is not None:
        mask = synth.padding_mask(x)
    if c.get("randmask") is not None:
        mask = synth.random_mask(c["B"], c["T"], c["randmask"])
    return sd, x, mask


def valid_rows(c, mask):
    """bool [B, N]: the non-padding queries (all of them without a mask; the class token is never padding)"""
    N = c["T"] + (1 if c.get("use_cls") else 0)
    v = np.ones((c["B"], N), dtype=bool)
    if mask is not None:
        v[:, N - c["T"]:] = ~mask.numpy().astype(bool)
    return v


def reductions64(P, valid):
    """float64 (received [.., B, H, N], entropy [.., B, H, N]) of maps P [.., B, H, N, N]; valid bool [B, N]"""
    P = np.asarray(P, dtype=np.float64)
    w = valid.astype(np.float64)[:, None, :, None]                       # [B, 1, N, 1] over the query axis
    received = (P * w).sum(axis=-2) / valid.sum(axis=1).astype(np.float64)[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(P > 0, P * np.log(P), 0.0)
    return received, -plogp.sum(axis=-1)
