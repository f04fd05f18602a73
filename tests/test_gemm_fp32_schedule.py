"""The k-loop schedule of the exact-fp32 Linear kernels, pinned in the gfx950 assembly (no GPU needed).

DESIGN.md section 5 (round 6): the k-loops of gemm_nt_128<*, 4, 0, 4, 0> and gemm_ln_rows<8, 0> read every LDS fragment
well ahead of its first use, carry no 64-bit address arithmetic and no branch.  The compiler is free to undo all of that
silently (it did, before the reads were pinned with sched_group_barrier: it sank them to the end of each group), so the
emitted loop is checked here: vs_kernels.hip is compiled to assembly with the library's own flags, the loop between the
k-tile barriers is cut out of each headline instantiation, and its instruction stream is inspected.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# MFMAs of the wave's own between a fragment's ds_read_b128 and the s_waitcnt lgkmcnt that covers it, for every read but
# the ones at the top of the loop (the k-tile's first fragments can only be read after the barrier).  One exact-fp32 MFMA
# occupies the matrix pipe for 64 cycles, so 4 of them are 256 cycles - a b128 LDS read returns within that when the
# array is shared with the block's other waves (an unloaded read takes about 128).  The stamped k-tile times of
# profiles/r06_gemm_fp32_kloop_after.txt were taken with the distances the kernels have (7 at least); the parent's
# distance was 0 (profiles/r06_gemm_fp32_kloop_before.txt), and this test fails on its assembly.
MIN_MFMA_DISTANCE = 4

HEADLINE = {      # mangled-name fragment: MFMAs per k-tile and wave
    "gemm_nt_128ILi1ELi4ELi0ELi4ELi0ELi0ELi32ELi0E": 128,      # fc1 (ReLU epilogue)
    "gemm_nt_128ILi3ELi4ELi0ELi4ELi0ELi0ELi32ELi0E": 128,      # QKV
    "gemm_nt_128ILi2ELi4ELi0ELi4ELi0ELi0ELi32ELi0E": 128,      # embedding (+ positional table)
    "gemm_ln_rowsILi8ELi0ELi0ELi0E": 64,                        # out-projection / fc2 + LayerNorm (16-wide k-tiles)
}


@pytest.fixture(scope="module")
def asm(vsa, tmp_path_factory):
    csrc = os.path.join(ROOT, "video-summarization_amd", "csrc")
    out = str(tmp_path_factory.mktemp("isa") / "vs_kernels.s")
    r = subprocess.run([vsa._lib.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I" + csrc,
                        "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                        os.path.join(csrc, "vs_kernels.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def _function(text, frag):
    """(instruction lines, vgprs, scratch bytes) of the kernel whose mangled name contains `frag`."""
    m = re.search(r"^(_Z\w*%s\w*):" % re.escape(frag), text, re.M)
    assert m, frag
    body = text[m.end():]
    body = body[:body.index(".Lfunc_end")]
    meta = text[m.end():]
    vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    sc = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
    lines = [l.split(";")[0].strip() for l in body.split("\n")]
    return [l for l in lines if l], vg, sc


def _kloop(lines, n_mfma):
    """The innermost loop that holds MFMAs and a barrier: from its label to its backward branch."""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if m and labels.get(m.group(1), i) < i:
            body = lines[labels[m.group(1)] + 1:i]
            if any(b.startswith("v_mfma") for b in body) and "s_barrier" in body:
                loops.append(body)
    assert loops, "no k-loop found"
    inner = min(loops, key=len)
    assert sum(b.startswith("v_mfma_f32_32x32x2_f32") for b in inner) == n_mfma
    return inner


def _read_distances(body):
    """For every ds_read_b128 after the loop's first MFMA: MFMAs between it and the s_waitcnt lgkmcnt(n) that covers it.
    LDS instructions return in order, so a wait for n covers all but the n youngest outstanding ones."""
    out, pending, mf, seen_mfma = [], [], 0, False
    for l in body:
        op = l.split()[0]
        if op.startswith("v_mfma"):
            mf += 1
            seen_mfma = True
        elif op.startswith("ds_"):
            pending.append((mf, op == "ds_read_b128" and seen_mfma))
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", l)
            if m:
                n = int(m.group(1))
                done, pending = (pending[:len(pending) - n], pending[len(pending) - n:]) if n else (pending, [])
                out += [mf - at for at, counted in done if counted]
    assert not any(counted for _, counted in pending), "a fragment read is never waited for inside the loop"
    return out


@pytest.mark.parametrize("frag", sorted(HEADLINE))
def test_kloop_of_headline_instantiation(asm, frag):
    lines, vgprs, scratch = _function(asm, frag)
    body = _kloop(lines, HEADLINE[frag])
    assert vgprs <= 256 and scratch == 0, (vgprs, scratch)
    ops = [l.split()[0] for l in body]
    assert not [o for o in ops if o.startswith("scratch_")]
    assert "v_lshl_add_u64" not in ops and "v_add_co_u32_e32" not in ops, "64-bit address arithmetic in the k-loop"
    assert not [o for o in ops if o.startswith("s_cbranch") or o.startswith("s_branch") or o.startswith("s_and_saveexec")]
    assert ops.count("s_barrier") == 1
    dist = _read_distances(body)
    reads_at_top = 0
    for o in ops:
        if o.startswith("v_mfma"):
            break
        reads_at_top += o == "ds_read_b128"
    assert reads_at_top + len(dist) == ops.count("ds_read_b128")
    print("%s: %d VGPRs, %d reads at the top, distances of the other %d: min %d" % (frag, vgprs, reads_at_top, len(dist), min(dist)))
    assert len(dist) >= ops.count("ds_read_b128") // 2
    assert min(dist) >= MIN_MFMA_DISTANCE, sorted(dist)[:8]


def test_linear_kernels_keep_their_place_in_the_code_object(asm):
    """the compiler emits the instantiations of a kernel template in the order vs_kernels.hip first names
    them.  With the same kernels in another order the 16-bit training step at 64 x 1024 measured 0.4 - 0.6 % slower
    (profiles/linear_pick_bench.txt), so name_gemm_kernels / name_ln_kernels name them first, in the order they had before the
    launchers dispatched over a pick.  tests/golden/vs_kernels_symbol_order.txt is that order: the `.amdhsa_kernel` symbols of the
    product build as the compiler wrote them.  A kernel that is added or removed on purpose changes the list; re-record it then."""
    with open(os.path.join(ROOT, "tests", "golden", "vs_kernels_symbol_order.txt")) as f:
        want = f.read().split()
    got = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    moved = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not moved, "first kernel out of place: position %d, expected %s, found %s" % moved[0]
