"""Resources and loop discipline of the one-launch layer tail, pinned in the gfx950 assembly (no GPU needed).

DESIGN.md section 5 (round 9): gemm_ln_rows_tail_qkv and gemm_ln_rows_tail_score are the two round-7 layer kernels as two
phases of one tile - out-projection + LayerNorm1 and the fc1 chunks, then fc2 over the hidden rows the block has just written, with the
accumulators still holding h1, LayerNorm2 and the QKV chunks or the score head.  That only pays with two blocks per CU: 256
registers without scratch, 80 KiB of LDS although the small vectors of both phases are resident.  The loops are those of
test_layer_fused_schedule.py (64 MFMAs per k-tile, 64 per step of a chunk), and the point of the kernel is in the assembly
too: between the first k-loop and the fc1 chunk loop - LayerNorm1 - nothing is stored to memory, and between the fc1 chunk
loop and the second k-loop no residual is fetched.
Modelled on test_layer_fused_schedule.py: vs_kernels.hip is compiled to assembly with the library's own flags.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEP = 64                       # MFMAs per wave between two barriers: a 16-wide k-tile, or one 32-wide step of a 128-column chunk
CHUNK = 8 * STEP + 4            # a chunk: 8 steps and the next chunk's 4 bias MFMAs
# kernel: MFMAs per wave of its loops, in program order
KERNELS = {"gemm_ln_rows_tail_qkv": [STEP, CHUNK, STEP, CHUNK], "gemm_ln_rows_tail_score": [STEP, CHUNK, STEP]}
STORES = ("global_store", "buffer_store", "flat_store")


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
    """(first line, last line) of every loop (label .. backward branch) that holds MFMAs and a barrier and no other such loop
    inside it, in program order."""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if m and labels.get(m.group(1), i) < i:
            lo = labels[m.group(1)]
            body = lines[lo + 1:i]
            if any(b.startswith("v_mfma") for b in body) and "s_barrier" in body:
                loops.append((lo, i))
    return sorted((lo, hi) for lo, hi in loops if not any(lo < lo2 and hi2 < hi for lo2, hi2 in loops))


def _mfmas_between_barriers(body):
    counts, n = [], 0
    for l in body:
        if l.split()[0] == "s_barrier":
            counts.append(n)
            n = 0
        elif l.startswith("v_mfma_f32_32x32x2_f32"):
            n += 1
    return counts, n


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
def test_every_loop_runs_64_mfmas_between_two_barriers(asm, frag):
    lines, _desc_, _ = _kernel(asm, frag)
    loops = _mfma_loops(lines)
    bodies = [lines[lo + 1:hi] for lo, hi in loops]
    assert [sum(b.startswith("v_mfma_f32_32x32x2_f32") for b in body) for body in bodies] == KERNELS[frag]
    for body, total in zip(bodies, KERNELS[frag]):
        counts, rest = _mfmas_between_barriers(body)
        if total == STEP:                   # a k-tile: its 64 MFMAs, then the barrier
            assert counts == [STEP] and rest == 0, (counts, rest)
        else:                               # a chunk: 8 steps of 64 with a barrier each, then the next chunk's bias MFMAs
            assert counts == [STEP] * 8 and rest == 4, (counts, rest)
        ops = [l.split()[0] for l in body]
        assert not [o for o in ops if o.startswith("s_cbranch") or o.startswith("s_branch") or o.startswith("s_and_saveexec")], \
            "a branch between two barriers"
        assert not [o for o in ops if o.startswith("scratch_")]


@pytest.mark.parametrize("frag", sorted(KERNELS))
def test_layernorm1_stores_nothing_and_fc2_fetches_no_residual(asm, frag):
    lines, _desc_, _ = _kernel(asm, frag)
    loops = _mfma_loops(lines)
    ln1 = lines[loops[0][1]:loops[1][0]]            # behind the first k-loop, up to the fc1 chunk loop: LayerNorm1
    assert len(ln1) > 200, len(ln1)                 # (the region is the epilogue, not an empty gap)
    assert not [l for l in ln1 if l.startswith(STORES)], "h1 is stored"
    # guarded stores may be laid out of line, behind the loops: the whole kernel holds LayerNorm2's 8 x 4 row stores and no more
    assert sum(l.startswith("global_store_dwordx4") for l in lines) == 32
    head2 = lines[loops[1][1]:loops[2][0]]          # behind the fc1 chunk loop, up to the second k-loop
    ops = [l.split()[0] for l in head2]
    assert not [o for o in ops if o.startswith("global_load") or o.startswith("flat_load")], "a residual is fetched in front of fc2"
    assert ops.count("buffer_load_dwordx4") == 6    # k-tile 0: four pieces of W2, two of the hidden rows
    # the hidden rows' loads come behind the wait for this wave's stores and the block's barrier; W2's come in front of them
    wait = [i for i, l in enumerate(head2) if l.startswith("s_waitcnt") and "vmcnt(0)" in l][0]
    bar = ops.index("s_barrier")
    loads = [i for i, o in enumerate(ops) if o == "buffer_load_dwordx4"]
    assert wait < bar and [i < wait for i in loads] == [True] * 4 + [False] * 2 and loads[4] > bar, (wait, bar, loads)


def test_the_same_regions_of_the_round_7_kernels_do_store_and_fetch(asm):
    """The detector of the test above sees what it looks for where it exists: layer_outproj_ln_fc1 stores h1 in its LayerNorm
    epilogue, layer_fc2_ln_qkv fetches its residual in front of its k-loop."""
    lines, _desc_, _ = _kernel(asm, "layer_outproj_ln_fc1")
    loops = _mfma_loops(lines)
    assert [l for l in lines[loops[0][1]:loops[1][0]] if l.startswith(STORES)]
    assert sum(l.startswith("global_store_dwordx4") for l in lines) == 32
    lines, _desc_, _ = _kernel(asm, "layer_fc2_ln_qkv")
    loops = _mfma_loops(lines)
    assert len([l for l in lines[:loops[0][0]] if l.startswith("global_load_dwordx4")]) >= 32
