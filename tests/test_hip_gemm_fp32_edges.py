"""Exact-fp32 tiled Linear kernels (gemm_nt_128, gemm_ln_rows) against float64 at awkward row counts.

These kernels stage their operand rows through a buffer descriptor that starts at the output tile's first row, with one
32-bit offset per staged row and the edge rows clamped once per tile.  The shapes here put the edge everywhere it can
go wrong: M below one tile, one row short of a tile, one row past a tile (256 k + 1, also at the row counts where the
launcher picks the 256x256 tiles on 8-wave blocks), N in {256, 768, 1024}, K in {256, 1024}.  The latency (skinny)
kernels are switched off so that every case runs the tiled kernels.  Bound: tests/tolerances.py FP32_TOL.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import tolerances as tol

pytestmark = pytest.mark.gpu

SMALL_M = (100, 255, 257, 513, 1000)            # 4-wave blocks, 128x128 tiles
WIDE_M = (16385, 65537)                         # 256 k + 1 where N = 1024 / every N gets the 8-wave 256x256 tiles


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def tiled(vsa):
    vsa._lib.set_option("VS_SKINNY_ROWS", 0)
    yield
    vsa._lib.set_option("VS_SKINNY_ROWS", -1)


def _operands(M, N, K):
    g = torch.Generator().manual_seed(7 * M + 3 * N + K)
    A = torch.randn(M, K, generator=g).to(_dev())
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(_dev())
    b = torch.randn(N, generator=g).to(_dev())
    return g, A, W, b


def _linear64(A, W, b):
    """float64 reference on the device, in row chunks."""
    W64, b64 = W.double(), b.double()
    return torch.cat([F.linear(A[i:i + 8192].double(), W64, b64) for i in range(0, A.shape[0], 8192)])


def _max_err(out, ref):
    assert torch.isfinite(out).all()
    return (out.double() - ref).abs().max().item()


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("N", [256, 768, 1024])
@pytest.mark.parametrize("M", SMALL_M + WIDE_M)
def test_tiled_linear_matches_float64(vsa, tiled, M, N, K):
    lib = vsa._lib.load()
    _, A, W, b = _operands(M, N, K)
    relu = 1 if N == 1024 else 0                 # fc1's epilogue at fc1's width
    ref = _linear64(A, W, b)
    if relu:
        ref = F.relu(ref)
    out = torch.full((M, N), float("nan"), device=_dev())
    vsa._lib.check(lib.vs_linear_f32(A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, relu, None, 0, _stream()))
    torch.cuda.synchronize()
    err = _max_err(out, ref)
    print("linear M=%d N=%d K=%d relu=%d: max |err| %.3e" % (M, N, K, relu, err))
    assert err < tol.FP32_TOL


@pytest.mark.parametrize("M", SMALL_M + (65537,))
def test_tiled_embedding_with_positional_table_matches_float64(vsa, tiled, M):
    """EPI_PE at the embedding's shape (N = 256, K = 1024): two videos of T frames, the second one cut short by the edge."""
    lib = vsa._lib.load()
    N, K = 256, 1024
    g, A, W, b = _operands(M, N, K)
    T = (M + 1) // 2
    pe = torch.randn(T, N, generator=g).to(_dev())
    ref = _linear64(A, W, b) + pe.double().repeat(2, 1)[:M]
    out = torch.full((M, N), float("nan"), device=_dev())
    vsa._lib.check(lib.vs_linear_f32(A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, 0, pe.data_ptr(), T, _stream()))
    torch.cuda.synchronize()
    err = _max_err(out, ref)
    print("embedding M=%d: max |err| %.3e" % (M, err))
    assert err < tol.FP32_TOL


@pytest.mark.parametrize("T", SMALL_M + (65537,))
def test_tiled_qkv_projection_matches_float64(vsa, tiled, T):
    """EPI_QKV (N = 768, K = 256, head-major output) with one video of T frames."""
    lib = vsa._lib.load()
    d, H = 256, 4
    _, h, W, b = _operands(T, 3 * d, d)
    ref = _linear64(h, W, b).view(1, T, 3, H, d // H).permute(2, 0, 3, 1, 4)
    out = torch.full((3, 1, H, T, d // H), float("nan"), device=_dev())
    vsa._lib.check(lib.vs_qkv_proj_f32(h.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), 1, T, d, H, _stream()))
    torch.cuda.synchronize()
    err = _max_err(out, ref)
    print("qkv T=%d: max |err| %.3e" % (T, err))
    assert err < tol.FP32_TOL


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("M", SMALL_M + (127, 129, 65537))
def test_linear_residual_layernorm_rows_matches_float64(vsa, tiled, M, K):
    """gemm_ln_rows<8, 0> (N = 256): out-projection (K = 256) and fc2 (K = 1024) with residual, LayerNorm and score head."""
    lib = vsa._lib.load()
    N = 256
    g, A, W, b = _operands(M, N, K)
    res = torch.randn(M, N, generator=g).to(_dev())
    gam, bet = (1 + 0.1 * torch.randn(N, generator=g)).to(_dev()), (0.1 * torch.randn(N, generator=g)).to(_dev())
    sw, sb = (torch.randn(1, N, generator=g) / math.sqrt(N)).to(_dev()), torch.randn(1, generator=g).to(_dev())
    y = F.layer_norm(_linear64(A, W, b) + res.double(), (N,), gam.double(), bet.double(), 1e-5)
    sc = F.linear(y, sw.double(), sb.double())
    out = torch.full((M, N), float("nan"), device=_dev())
    scores = torch.full((M, 1), float("nan"), device=_dev())
    vsa._lib.check(lib.vs_linear_residual_layernorm_f32(
        A.data_ptr(), W.data_ptr(), b.data_ptr(), res.data_ptr(), gam.data_ptr(), bet.data_ptr(), out.data_ptr(), M, N, K,
        sw.data_ptr(), sb.data_ptr(), 1, 0, scores.data_ptr(), _stream()))
    torch.cuda.synchronize()
    e1, e2 = _max_err(out, y), _max_err(scores, sc)
    print("linear+LN M=%d K=%d: max |err| out %.3e score %.3e" % (M, K, e1, e2))
    assert e1 < tol.FP32_TOL and e2 < tol.FP32_TOL
