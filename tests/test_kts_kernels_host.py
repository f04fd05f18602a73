"""CPU (no GPU): the cosine / rbf kernels of KTS - exports, the argument checks of the new C entry points, workspace sizes,
the Python surface's errors, and the float64 definitions (tests/kts_kernels_ref.py + tests/kts_ref.py) against the
reference's results stored in tests/golden/kts_kernels_golden.npz."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import kts_kernels_ref as kk
import kts_ref

GOLD = os.path.join(GOLDEN, "kts_kernels_golden.npz")
NEW = ("vs_kts_gram_workspace_bytes", "vs_kts_gram", "vs_kts_workspace_bytes_k", "vs_kts_segment_k", "vs_kts_eval_score")


def golden():
    z = np.load(GOLD)
    return json.loads(str(z["cases"])), z


CASES, _ = golden()


def _arr(v, ct):
    return (ct * len(v))(*v)


def test_every_new_symbol_is_exported_and_declared(vsa):
    vsa._lib.build()
    lib = vsa._lib.load()
    for name in NEW:
        assert name in vsa._lib.SEGMENT_EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert (vsa._lib.VS_KTS_GRAM_DOT, vsa._lib.VS_KTS_GRAM_COSINE, vsa._lib.VS_KTS_GRAM_RBF) == (0, 1, 2)
    assert C.sizeof(vsa._lib.KtsKernel) == 16
    seg = vsa.segmentation
    for name in ("gram", "eval_score", "eval_cost", "estimate_vmax", "centering", "kts_seg", "kts_seg_batch"):
        assert name in seg.__all__ and callable(getattr(seg, name)), name


def _kern(vsa, kind=1, reserved=0, gamma=0.0):
    return vsa._lib.KtsKernel(kind, reserved, gamma)


BAD_KERNELS = [dict(kind=3), dict(kind=-1), dict(kind=1, reserved=1), dict(kind=2, gamma=float("nan")),
               dict(kind=2, gamma=float("inf")), dict(kind=2, gamma=0.0), dict(kind=2, gamma=-1.0)]
DEV = C.c_void_p(16)            # a non-NULL "device" pointer that a refused call never touches


def _segment_k(lib, kern, inp=0, cu=(0, 100), ncp=(3,), ws=1 << 30):
    B = len(cu) - 1
    cps, n_cps, scores = (C.c_int64 * 64)(), (C.c_int32 * 8)(), (C.c_double * 64)()
    return lib.vs_kts_segment_k(DEV, inp, 64, _arr(cu, C.c_int32), B, _arr(ncp, C.c_int32), None, None, _arr([1.0] * B, C.c_double),
                                None, 2, kern, cps, n_cps, scores, DEV, ws, None)


def test_invalid_kernels_are_refused_by_every_entry_point_without_a_gpu(vsa):
    lib, INVALID = vsa._lib.load(), vsa._lib.VS_ERR_INVALID
    cu, ncp = _arr([0, 100], C.c_int32), _arr([3], C.c_int32)
    out = (C.c_double * 1)()
    for kw in BAD_KERNELS:
        k = C.byref(_kern(vsa, **kw))
        assert _segment_k(lib, k) == INVALID and lib.vs_last_error(), kw
        assert lib.vs_kts_gram(DEV, 64, cu, 1, k, DEV, DEV, 1 << 30, None) == INVALID, kw
        assert lib.vs_kts_workspace_bytes_k(cu, 1, 64, 0, ncp, 2, k) == 0, kw
        assert lib.vs_kts_eval_score(DEV, 0, 64, k, cu, 1, _arr([10, 20, 30], C.c_int64), ncp, out, DEV, 1 << 30, None) == INVALID, kw
    assert _segment_k(lib, None) == INVALID                                      # kern is required
    assert lib.vs_kts_gram(DEV, 64, cu, 1, None, DEV, DEV, 1 << 30, None) == INVALID
    good = C.byref(_kern(vsa, 2, 0, 0.5))
    for inp in (vsa._lib.VS_KTS_KERNEL_F32, vsa._lib.VS_KTS_KERNEL_F64):          # a kernel matrix has its kernel already
        assert _segment_k(lib, good, inp=inp) == INVALID
        assert b"kernel" in lib.vs_last_error()
        assert lib.vs_kts_workspace_bytes_k(cu, 1, 64, inp, ncp, 2, good) == 0
    # the checks of vs_kts_segment hold for the _k form too, and a short workspace is its own status
    assert _segment_k(lib, good, cu=(0, 10), ncp=(10,)) == INVALID
    assert _segment_k(lib, good, cu=(1, 100)) == INVALID
    assert _segment_k(lib, good, ws=16) == vsa._lib.VS_ERR_WORKSPACE
    assert lib.vs_kts_gram(DEV, 0, cu, 1, good, DEV, DEV, 1 << 30, None) == INVALID          # d = 0
    assert lib.vs_kts_gram(DEV, 64, cu, 0, good, DEV, DEV, 1 << 30, None) == INVALID         # batch = 0
    assert lib.vs_kts_gram(DEV, 64, cu, 1, good, DEV, DEV, 16, None) == vsa._lib.VS_ERR_WORKSPACE
    assert lib.vs_kts_gram_workspace_bytes(_arr([0, 10, 5], C.c_int32), 2, 64) == 0


def test_invalid_change_points_are_refused_without_a_gpu(vsa):
    lib, INVALID = vsa._lib.load(), vsa._lib.VS_ERR_INVALID
    cu = _arr([0, 50, 100], C.c_int32)
    out = (C.c_double * 2)()

    def call(cps, n_cps, inp=2, kern=None):
        return lib.vs_kts_eval_score(DEV, inp, 0 if inp else 64, kern, cu, 2, _arr(cps, C.c_int64), _arr(n_cps, C.c_int32), out,
                                     DEV, 16, None)

    for cps, n_cps in [([0, 10], [2, 0]), ([10, 50], [2, 0]), ([10, 10], [2, 0]), ([20, 10], [2, 0]), ([-3], [1, 0]),
                       ([10, 20, 50], [2, 1]), ([10, 20, 0], [2, 1]), ([5], [0, -1])]:
        for inp in (0, 1, 2):
            assert call(cps, n_cps, inp) == INVALID and lib.vs_last_error(), (cps, n_cps, inp)
    # valid change points pass the checks and stop at the workspace size: still no device access
    assert call([10, 49, 1, 49], [2, 2]) == vsa._lib.VS_ERR_WORKSPACE
    assert call([10, 49, 1, 49], [2, 2], inp=0, kern=C.byref(_kern(vsa, 1))) == vsa._lib.VS_ERR_WORKSPACE


def test_workspace_sizes_are_non_zero_and_grow_with_n(vsa):
    lib = vsa._lib.load()
    k = C.byref(_kern(vsa, 1))
    last_g = last_s = 0
    for n in (1, 64, 65, 1000, 4000):
        cu, ncp = _arr([0, n], C.c_int32), _arr([min(5, n - 1)], C.c_int32)
        g = lib.vs_kts_gram_workspace_bytes(cu, 1, 1024)
        s = lib.vs_kts_workspace_bytes_k(cu, 1, 1024, 0, ncp, 2, k)
        assert g >= n * 8 and g > 0 and s >= lib.vs_kts_workspace_bytes(cu, 1, 1024, 0, ncp, 2) + n * 8
        assert g >= last_g and s > last_s
        last_g, last_s = g, s
    assert last_g >= 4000 * 8 > lib.vs_kts_gram_workspace_bytes(_arr([0, 1], C.c_int32), 1, 1024)
    # a batch: the row norms of every video, a descriptor per video
    assert lib.vs_kts_gram_workspace_bytes(_arr([0, 100, 300, 301], C.c_int32), 3, 7) >= 301 * 8 + 3 * 24


def test_python_surface_refuses_unknown_kernels_and_stray_gammas(vsa, monkeypatch):
    seg = vsa.segmentation
    x = np.ones((10, 8), np.float32)
    for fn in (lambda **kw: seg.kts_seg(x, 2, 1.0, **kw), lambda **kw: seg.kts_seg_batch([x, x], 2, 1.0, **kw),
               lambda **kw: seg.gram(x, **kw), lambda **kw: seg.gram([x, x], **kw)):
        with pytest.raises(NotImplementedError):
            fn(kernel="chi2")
        for kernel in ("dot", "cosine"):
            with pytest.raises(ValueError, match="gamma"):
                fn(kernel=kernel, gamma=0.5)
        for gamma in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="gamma"):
                fn(kernel="rbf", gamma=gamma)
    with pytest.raises(ValueError, match="gamma"):
        seg.kts_seg_batch([x], 2, 1.0, gamma=1.0)                                # the default kernel is "dot"
    # the new kernels are device code like the rest: no CPU path
    monkeypatch.setattr(seg.torch.cuda, "is_available", lambda: False)
    for kw in (dict(kernel="cosine"), dict(kernel="rbf"), dict(kernel="rbf", gamma=0.1)):
        with pytest.raises(RuntimeError, match="HIP kernels only"):
            seg.kts_seg(x, 2, 1.0, **kw)
        with pytest.raises(RuntimeError, match="HIP kernels only"):
            seg.gram(x, **kw)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        seg.eval_score(np.eye(10), [3])
    with pytest.raises(NotImplementedError, match="rbf"):                    # not implemented off the device, like the reference
        seg.kts_seg_batch([x, x], 2, 1.0, kernel="rbf")
    with pytest.raises(RuntimeError) as e:
        seg.kts_seg(x, 2, 1.0)                                               # "dot" keeps its own error
    assert not isinstance(e.value, NotImplementedError)
    # eval_cost is host arithmetic in the reference's order; centering is plain array code
    K = kk.kernel64(x + np.arange(10, dtype=np.float32)[:, None], "rbf", 0.01)
    assert seg.eval_cost(K, [3, 7], 2.5, 0.4) == 2.5 / 10.0 + (0.4 * 2 / (2.0 * 10)) * (np.log(10.0 / 2) + 1)
    Kc = seg.centering(K)
    assert np.abs(Kc.sum(0)).max() < 1e-12 and np.abs(Kc.sum(1)).max() < 1e-12
    assert np.abs(seg.centering(seg.torch.from_numpy(K)).numpy() - Kc).max() < 1e-15


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_definitions_reproduce_the_reference_goldens(name):
    """Anchors tests/kts_kernels_ref.kernel64 + tests/kts_ref to the reference: the float64 K rebuilt from the stored
    features gives the golden change points, costs, eval_score and estimate_vmax."""
    c, z = CASES[name], golden()[1]
    x = z["x/" + c["x"]]
    assert x.dtype == np.float32 and x.shape[0] <= 256 and x.shape[1] <= 100
    K = kk.kernel64(x, c["kind"], c["gamma"])
    assert np.abs(K - K.T).max() <= 4e-16 and (np.diag(K) == 1).all() and np.abs(K).max() <= 1
    cps, costs, _, margin = kts_ref.kts_segmentation(K, c["ncp"], c["vmax"])
    np.testing.assert_array_equal(cps, z[name + "/cps"])
    assert np.abs(costs - z[name + "/costs"]).max() <= 1e-12 * np.abs(z[name + "/costs"]).max()
    assert 0 < len(cps) < c["ncp"] and margin >= 1000 * c["cost_err32"] and abs(margin - c["margin"]) <= 1e-9 * margin
    score = kts_ref.objective(K, cps)
    assert abs(score - float(z[name + "/eval_score"])) <= 1e-12 * abs(score)
    n0 = c["stable"]
    vmax_est = kts_ref.objective(K[:n0, :n0], []) / n0
    assert abs(vmax_est - float(z[name + "/estimate_vmax"])) <= 1e-12 * abs(vmax_est)
    # the fp32-Gram kernel chooses the same change points: the generator's condition
    K32 = kk.kernel64(x, c["kind"], c["gamma"], gram32=True)
    np.testing.assert_array_equal(kts_ref.kts_segmentation(K32, c["ncp"], c["vmax"])[0], cps)
