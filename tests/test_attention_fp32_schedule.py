"""The steady-state tile loop of the exact-fp32 attention kernel, pinned in the gfx950 assembly (no GPU needed).

DESIGN.md section 5 (round 8): the fp32 MFMA shares its issue port with ordinary vector instructions, so the loop of
attn_fwd_pipe<64, false, 8, false, 0> is written to issue as few of them as possible: the row bias rides in as the C operand of
a block's first S' MFMA (no bias MFMA), a block's maximum is a tree of three-input maxima, and the loop runs two tiles per
iteration so that the LDS buffer parity and every address that follows from it are immediates.  The compiler is free to undo
any of that silently, so the emitted loop is counted here: vs_attention.hip is compiled to assembly with the library's own
flags and the loop between the tile barriers is cut out of the headline instantiation.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "attn_fwd_pipeILi64ELb0ELi8ELb0ELi0EE"       # <DH 64, no mask, 8 waves, padded batch, no stamps>
MFMA_PER_TILE = 128                                     # 2 blocks of 32 keys x (32 S' + 32 P.V)
MAX_VALU_PER_TILE = 105                                 # non-MFMA vector instructions per 128 MFMAs


@pytest.fixture(scope="module")
def loop(vsa, tmp_path_factory):
    csrc = os.path.join(ROOT, "video-summarization_amd", "csrc")
    out = str(tmp_path_factory.mktemp("isa") / "vs_attention.s")
    r = subprocess.run([vsa._lib.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I" + csrc,
                        "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                        os.path.join(csrc, "vs_attention.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(out).read()
    m = re.search(r"^(_Z\w*%s\w*):" % re.escape(HEADLINE), text, re.M)
    assert m, HEADLINE
    body = text[m.end():]
    body = body[:body.index(".Lfunc_end")]
    meta = text[m.end():]
    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
    lines = [l.split(";")[0].strip() for l in body.split("\n")]
    return [l for l in lines if l], vgprs, scratch


def _steady_loop(lines):
    """(first, last) line index of the steady-state loop: the shortest span from a label to a conditional backward branch
    that holds MFMAs and a barrier (the fix-up blocks may lie inside the span or after it)."""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if m and labels.get(m.group(1), i) < i:
            a = labels[m.group(1)]
            if any(b.startswith("v_mfma") for b in lines[a:i]) and "s_barrier" in lines[a:i]:
                loops.append((a, i))
    assert loops, "no tile loop found"
    return min(loops, key=lambda s: s[1] - s[0])


def _main_path(lines, first, last):
    """The instructions the loop executes when no fix-up is taken: from the loop's label, follow fall-through; a forward
    conditional branch inside the loop is a fix-up exit and is not taken, an unconditional one is followed.  Returns
    (instructions, conditional branches passed)."""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    path, exits, i, steps = [], [], first, 0
    while i != last:
        steps += 1
        assert steps < 100000 and first <= i <= last, "the loop's main path leaves the loop"
        l = lines[i]
        if l.endswith(":"):
            i += 1
            continue
        m = re.match(r"s_branch\s+(\S+)", l)
        if m:
            i = labels[m.group(1)]
            continue
        if l.startswith("s_cbranch"):
            exits.append(i)
        path.append(l)
        i += 1
    return path, exits


def _fixup_exit(lines, at, first, last):
    """A conditional branch of the main path is a fix-up exit if its target block is the rare path: it holds no MFMA and
    no barrier before it jumps back into the loop."""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    i = labels[re.match(r"s_cbranch_\w+\s+(\S+)", lines[at]).group(1)]
    for _ in range(400):
        l = lines[i]
        if l.startswith("v_mfma") or l == "s_barrier":
            return False
        if re.match(r"s_branch\s+(\S+)", l):
            return first <= labels[re.match(r"s_branch\s+(\S+)", l).group(1)] <= last
        i += 1
    return False


def test_steady_loop_of_headline_instantiation(loop):
    lines, vgprs, scratch = loop
    assert vgprs <= 256 and scratch == 0, (vgprs, scratch)
    first, last = _steady_loop(lines)
    path, exits = _main_path(lines, first, last)
    ops = [l.split()[0] for l in path]
    mfma = sum(o.startswith("v_mfma_f32_32x32x2_f32") for o in ops)
    assert mfma == sum(o.startswith("v_mfma") for o in ops)
    assert mfma in (MFMA_PER_TILE, 2 * MFMA_PER_TILE), mfma
    tiles = mfma // MFMA_PER_TILE
    valu = [o for o in ops if o.startswith("v_") and not o.startswith("v_mfma")]
    lds = [o for o in ops if o.startswith("ds_")]
    print("%d VGPRs; per tile: %d MFMAs, %.1f other vector instructions, %.1f LDS instructions (%d tile(s) per iteration)"
          % (vgprs, mfma // tiles, len(valu) / tiles, len(lds) / tiles, tiles))
    hist = {}
    for o in valu:
        hist[o] = hist.get(o, 0) + 1
    print(sorted(hist.items(), key=lambda kv: -kv[1]))
    assert len(valu) <= MAX_VALU_PER_TILE * tiles, len(valu) / tiles
    assert not [o for o in ops if o.startswith("scratch_")]
    assert ops.count("s_barrier") == 2 * tiles
    # no branch between the loop's barriers other than the fix-up exits (one per 32-key block)
    assert not [o for o in ops if o.startswith("s_and_saveexec") or o.startswith("s_setpc")]
    assert len(exits) <= 2 * tiles, [lines[i] for i in exits]
    for at in exits:
        assert _fixup_exit(lines, at, first, last), lines[at]
