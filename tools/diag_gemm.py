#!/usr/bin/env python3
"""Diagnostic: where does a k-tile iteration of the persistent projection GEMM spend its cycles?
Runs the fc1-shaped GEMM (M=65536, N=1024, K=256) in the stamped DIAG build and prints the shares.
Never part of a product run; see cdna guide §7 'In-kernel stamps'.

    diag_gemm.py [M N K]            the 4-wave / 128-column forms (VS_DIAG_MODE, VS_DIAG_NWM, VS_DIAG_PREC)
    diag_gemm.py M N K kloop        the headline exact-fp32 form gemm_nt_128<*, 4, *, 4> (256x256 tiles, 8 waves):
                                    cycles per k-tile, barrier wait per wave, epilogue share
    diag_gemm.py M 256 K kloop-ln   the same stamps in gemm_ln_rows<8, 0> (out-projection / fc2 + LayerNorm)"""
import ctypes as C
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("video-summarization_amd")
# the stamped instantiations live in the diagnostic build only (libvsscore_diag.so, -DVS_WITH_DIAG)
os.environ["VS_LIBRARY"] = pkg._lib.build(diag=True) if not os.path.exists(pkg._lib.DIAG_LIB_PATH) else pkg._lib.DIAG_LIB_PATH
lib = pkg._lib.load()
lib.vs_diag_gemm.restype = C.c_int
lib.vs_diag_gemm.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]

M, N, K = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (65536, 1024, 256)))
dev = torch.device("cuda:0")
A = torch.randn(M, K, device=dev)
W = torch.randn(N, K, device=dev) / K ** 0.5
b = torch.randn(N, device=dev)
Cc = torch.empty(M, N, device=dev)
st = torch.cuda.current_stream().cuda_stream


def run(grid, diag):
    mode = int(os.environ.get("VS_DIAG_MODE", "3"))
    mode = 3 if mode == 1 else mode
    g = grid if grid > 0 else 512
    dbuf = torch.zeros(g * 4 * 8, dtype=torch.int64, device=dev)
    dp = dbuf.data_ptr() if mode in (2, 3) else None       # modes 2/3 time the diagnostic build itself
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        pkg._lib.check(lib.vs_diag_gemm(A.data_ptr(), W.data_ptr(), b.data_ptr(), Cc.data_ptr(), M, N, K, grid, dp, st))
    e0.record()
    for _ in range(10):
        pkg._lib.check(lib.vs_diag_gemm(A.data_ptr(), W.data_ptr(), b.data_ptr(), Cc.data_ptr(), M, N, K, grid, dp, st))
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    print("grid %4d: %.4f ms  %.1f TFLOP/s" % (grid, ms, 2.0 * M * N * K / ms / 1e9))
    if mode in (2, 3):
        d = dbuf.view(g * 4, 8).double().cpu()
        cyc = d[:, 5].median().item()
        mf = 2.0 * M * N * K / 4096 / (256 * 4)          # MFMAs per SIMD
        t0, t1 = d[:, 3], d[:, 4]
        base = t0.min()
        print("   mode %d: cycles/wave min %.0f med %.0f max %.0f" % (mode, d[:, 5].min().item(), cyc, d[:, 5].max().item()))
        print("   wall (100 MHz ticks -> us): wave start min %.1f med %.1f max %.1f | wave end min %.1f med %.1f max %.1f | kernel %.1f us" % (
            0.0, ((t0 - base).median() / 100).item(), ((t0 - base).max() / 100).item(),
            ((t1 - base).min() / 100).item(), ((t1 - base).median() / 100).item(), ((t1 - base).max() / 100).item(), ms * 1e3))
        ends = ((t1 - base) / 100)[::4]          # one wave per block
        hist = torch.histc(ends, bins=12, min=ends.min().item(), max=ends.max().item())
        print("   block end-time histogram (%.0f..%.0f us): %s" % (ends.min().item(), ends.max().item(), [int(x) for x in hist.tolist()]))
        # do blocks b and b+256 (likely co-resident) pair up as early/late?
        if g == 512:
            e = ends.view(2, 256)
            print("   blocks 0-255 end med %.1f us, blocks 256-511 end med %.1f us; |pair difference| med %.1f us" % (
                e[0].median().item(), e[1].median().item(), (e[0] - e[1]).abs().median().item()))
        life = ((t1 - t0) / 100)
        print("   wave lifetime us: min %.1f med %.1f max %.1f -> in-wave clock %.2f GHz; MFMA-busy share of lifetime at 2 waves/SIMD = %.3f" % (
            life.min().item(), life.median().item(), life.max().item(), cyc / life.median().item() / 1e3,
            64.0 * (2.0 * M * N * K / 4096 / (g * 4)) * (g // 256) / cyc))
        return
    if diag:
        g = grid if grid > 0 else 512
        d = torch.zeros(g * 4 * 8, dtype=torch.int64, device=dev)
        pkg._lib.check(lib.vs_diag_gemm(A.data_ptr(), W.data_ptr(), b.data_ptr(), Cc.data_ptr(), M, N, K, grid, d.data_ptr(), st))
        torch.cuda.synchronize()
        d = d.view(g * 4, 8).double().cpu()
        names = ["issue_loads", "ds_read+mfma", "epilogue", "vmcnt+ds_write", "barrier"]
        tot = d[:, 5].mean().item()
        kt = d[:, 6].mean().item()
        print("   stamped build: mean cycles/wave %.0f over %.0f k-tiles = %.0f cycles per k-tile (64 MFMAs = 4096 busy)" % (tot, kt, tot / kt))
        for i, n in enumerate(names):
            print("   %-16s %6.1f %%   %7.0f cycles/k-tile   (min %.0f max %.0f per wave)" % (
                n, 100 * d[:, i].mean().item() / tot, d[:, i].mean().item() / kt, (d[:, i] / d[:, 6]).min().item(), (d[:, i] / d[:, 6]).max().item()))
        tb = d[:, 7]
        print("   start skew across waves: %.0f cycles" % (tb.max() - tb.min()).item())


def run_kloop(ln):
    """Stamped build of a headline instantiation on its product grid, beside the unstamped product kernel."""
    os.environ["VS_DIAG_MODE"] = "3"
    if ln:
        os.environ["VS_DIAG_KERNEL"] = "ln"
        wpb, mf_tile = 4, 4 * 8 * 4                 # waves per block; MFMAs per wave and 16-wide k-tile: 4 steps x 8 column tiles
        blocks = min(512, (M + 127) // 128)
    else:
        os.environ["VS_DIAG_NJ"] = "4"
        wpb, mf_tile = 8, 128
        blocks = min(256, (M + 255) // 256 * (N // 256))
    call = lambda dp: pkg._lib.check(lib.vs_diag_gemm(A.data_ptr(), W.data_ptr(), b.data_ptr(), Cc.data_ptr(), M, N, K, 0, dp, st))
    blocks = max(blocks, 1024)                      # head-room: the library sizes the grid from the CU count
    dbuf = torch.zeros(blocks * wpb * 8, dtype=torch.int64, device=dev)
    for name, dp in (("product kernel", None), ("stamped build", dbuf.data_ptr())):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            call(dp)
        e0.record()
        for _ in range(10):
            call(dp)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        print("%-15s %s M=%d N=%d K=%d: %.4f ms  %.1f TFLOP/s (%.3f of 157.3)" % (
            name, "gemm_ln_rows<8,0>" if ln else "gemm_nt_128<1,4,*,4>", M, N, K, ms, 2.0 * M * N * K / ms / 1e9, 2.0 * M * N * K / ms / 1e9 / 157.3))
    d = dbuf.view(blocks * wpb, 8).double().cpu()
    d = d[d[:, 6] > 0]
    kt = d[:, 6]
    issue = 2.0 * 64 * mf_tile                      # cycles of pure MFMA issue per k-tile for the SIMD's two waves
    per = d[:, 5] / kt
    bar = d[:, 0] / kt
    print("   waves %d, k-tiles per wave med %.0f; cycles per k-tile and wave: mean %.0f med %.0f min %.0f max %.0f  (pure MFMA issue of the SIMD's two waves: %.0f -> %.3f)" % (
        d.shape[0], kt.median().item(), per.mean().item(), per.median().item(), per.min().item(), per.max().item(), issue, issue / per.mean().item()))
    print("   barrier wait per k-tile and wave: mean %.0f med %.0f min %.0f max %.0f cycles (%.1f %% of the wave's time)" % (
        bar.mean().item(), bar.median().item(), bar.min().item(), bar.max().item(), 100 * d[:, 0].sum().item() / d[:, 5].sum().item()))
    w = torch.arange(d.shape[0]) % wpb
    print("   barrier wait by wave of the block (mean cycles per k-tile): " + "  ".join(
        "w%d %.0f" % (i, bar[w == i].mean().item()) for i in range(wpb)))
    half = wpb // 2
    print("   first-dispatched half %.0f | second half %.0f ; share of waves waiting < 1/4 of the mean: %.2f, > 2x the mean: %.2f" % (
        bar[w < half].mean().item(), bar[w >= half].mean().item(), (bar < bar.mean() / 4).double().mean().item(), (bar > 2 * bar.mean()).double().mean().item()))
    hist = torch.histc(bar, bins=10, min=0, max=bar.max().item())
    print("   histogram of per-wave barrier wait (0..%.0f cycles per k-tile): %s" % (bar.max().item(), [int(x) for x in hist.tolist()]))
    print("   epilogue%s: %.1f %% of the wave's time (%.0f cycles per output tile)" % (
        " (LayerNorm + stores)" if ln else "", 100 * d[:, 1].sum().item() / d[:, 5].sum().item(), (d[:, 1] * (K // (16 if ln else 32)) / kt).mean().item()))
    if ln:
        print("   tile prologue (C-in and first k-tile loads, 2 barriers): %.1f %% (%.0f cycles per output tile)" % (
            100 * d[:, 2].sum().item() / d[:, 5].sum().item(), (d[:, 2] * (K // 16) / kt).mean().item()))


if len(sys.argv) > 4 and sys.argv[4].startswith("kloop"):
    run_kloop(sys.argv[4] == "kloop-ln")
    sys.exit(0)
for grid in ((256,) if os.environ.get('VS_DIAG_NWM') == '4' else (512, 256)):
    run(grid, True)
