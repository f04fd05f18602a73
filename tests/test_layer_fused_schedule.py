"""Resources and loop discipline of the exact-fp32 layer kernels, pinned in the gfx950 assembly (no GPU needed).

DESIGN.md section 5 (round 7): layer_outproj_ln_fc1 and layer_fc2_ln_qkv are a gemm_ln_rows<8, 0> tile followed by a
register-fed product - the wave's 32 normalised rows (128 registers) beside one 128-column chunk of accumulators (64).
That only pays with two blocks per CU, so the kernels must fit 256 registers without scratch and 80 KiB of LDS; and their
loops keep the round-6 discipline: no 64-bit address arithmetic beside the MFMAs and no branch between two barriers (the
chunk stores go through a buffer descriptor whose range check drops the rows past M, instead of a guarded store).
Modelled on test_gemm_fp32_schedule.py: vs_kernels.hip is compiled to assembly with the library's own flags.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel: (chunks of the register-fed product, MFMAs per wave in its chunk loop: 8 steps x 64 + the next chunk's 4 bias MFMAs)
KERNELS = {"layer_outproj_ln_fc1": (8, 8 * 64 + 4), "layer_fc2_ln_qkv": (6, 8 * 64 + 4)}
MIN_MFMA_DISTANCE = 4           # as test_gemm_fp32_schedule.py: MFMAs between a fragment's read and the wait that covers it


@pytest.fixture(scope="module")
def asm(vsa, tmp_path_factory):
    csrc = os.path.join(ROOT, "video-summarization_amd", "csrc")
    out = str(tmp_path_factory.mktemp("isa") / "vs_kernels.s")
    r = subprocess.run([vsa._lib.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I" + csrc,
                        "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                        os.path.join(csrc, "vs_kernels.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def _kernel(text, frag):
    """(instruction lines, the kernel's .amdhsa_* descriptor, scratch bytes) of the kernel whose mangled name contains `frag`."""
    m = re.search(r"^(_Z\w*%s\w*):" % re.escape(frag), text, re.M)
    assert m, frag
    name = m.group(1)
    body = text[m.end():]
    end = body.index(".Lfunc_end")
    sc = int(re.search(r"; ScratchSize: (\d+)", body[end:]).group(1))
    desc = text[text.index(".amdhsa_kernel " + name):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    lines = [l.split(";")[0].strip() for l in body[:end].split("\n")]
    return [l for l in lines if l], desc, sc


def _desc(desc, key):
    return int(re.search(r"\.amdhsa_%s (\d+)" % key, desc).group(1))


def _mfma_loops(lines):
    """Every loop (label .. backward branch) that holds MFMAs and a barrier and no other such loop inside it."""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if m and labels.get(m.group(1), i) < i:
            lo = labels[m.group(1)]
            body = lines[lo + 1:i]
            if any(b.startswith("v_mfma") for b in body) and "s_barrier" in body:
                loops.append((lo, i, body))
    return [b for lo, hi, b in loops if not any(lo < lo2 and hi2 < hi for lo2, hi2, _ in loops)]


@pytest.mark.parametrize("frag", sorted(KERNELS))
def test_resources_allow_two_blocks_per_cu(asm, frag):
    lines, desc, scratch = _kernel(asm, frag)
    vgprs, lds = _desc(desc, "next_free_vgpr"), _desc(desc, "group_segment_fixed_size")
    print("%s: %d VGPRs, %d B scratch, %d B LDS" % (frag, vgprs, scratch, lds))
    assert vgprs <= 256
    assert scratch == 0 and _desc(desc, "private_segment_fixed_size") == 0
    assert not [l for l in lines if l.startswith("scratch_")]
    assert lds <= 81920


@pytest.mark.parametrize("frag", sorted(KERNELS))
def test_mfma_loops_carry_no_wide_address_arithmetic_and_no_branch(asm, frag):
    lines, _desc_, _ = _kernel(asm, frag)
    loops = _mfma_loops(lines)
    per_loop = sorted(sum(b.startswith("v_mfma_f32_32x32x2_f32") for b in body) for body in loops)
    # the k-loop of the gemm_ln_rows tile (64 MFMAs per 16-wide k-tile) and the chunk loop of the register-fed product
    assert per_loop == [64, KERNELS[frag][1]], per_loop
    for body in loops:
        ops = [l.split()[0] for l in body]
        assert "v_lshl_add_u64" not in ops and "v_add_co_u32_e32" not in ops, "64-bit address arithmetic in an MFMA loop"
        assert not [o for o in ops if o.startswith("s_cbranch") or o.startswith("s_branch") or o.startswith("s_and_saveexec")], \
            "a branch between two barriers"
        assert not [o for o in ops if o.startswith("scratch_")]
    chunk = max(loops, key=len)
    ops = [l.split()[0] for l in chunk]
    assert ops.count("s_barrier") == 8                  # one per step of 64 MFMAs
    # per step: 16 fragment reads; the chunk's way out: 16 transposition reads behind the last barrier, 16 full-line stores
    assert ops.count("buffer_store_dwordx4") == 16 and ops.count("buffer_load_dwordx4") == 8 * 4
    # every fragment read of a step but its first two is issued at least MIN_MFMA_DISTANCE MFMAs ahead of the wait that covers it
    steps, cur = [], []
    for l in chunk:
        if l.split()[0] == "s_barrier":
            steps.append(cur)
            cur = []
        else:
            cur.append(l)
    assert len(steps) == 8
    for si, step in enumerate(steps):
        dist, pending, mf, seen = [], [], 0, False
        for l in step:
            op = l.split()[0]
            if op.startswith("v_mfma"):
                mf += 1
                seen = True
            elif op.startswith("ds_"):
                pending.append((mf, op == "ds_read_b128" and seen))
            elif op == "s_waitcnt":
                m = re.search(r"lgkmcnt\((\d+)\)", l)
                if m:
                    n = int(m.group(1))
                    done, pending = (pending[:len(pending) - n], pending[len(pending) - n:]) if n else (pending, [])
                    dist += [mf - at for at, counted in done if counted]
        assert len(dist) >= 8, (si, dist)
        assert min(dist) >= MIN_MFMA_DISTANCE, (si, sorted(dist)[:8])
