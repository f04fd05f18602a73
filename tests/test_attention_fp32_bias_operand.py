"""The C operand of attn_fwd_pipe's hand-written MFMA stays untouched while the MFMA reads it (no GPU needed).

DESIGN.md section 5 (round 8): the first S' MFMA of a 32-key block takes the row bias as its C operand and writes a register
block of its own; it is written as the instruction itself, so the compiler does not know that it is an MFMA and that it reads
its C registers over 16 passes.  A first version let the compiler hand those registers to the next instruction where they
held a temporary copy of the bias: the masked head-dim-32 kernels then returned wrong, run-to-run different results
(tests/test_hip_attention_maps.py::test_probs_kernel_against_float64[97-32]).  The kernel now keeps the operand alive until
the next MFMA has issued; this test reads every instantiation's assembly and checks that nothing writes a C register of a
hand-written MFMA before the next MFMA.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITES = re.compile(r"(v_\w+|ds_read\w*|buffer_load\w*|global_load\w*|scratch_load\w*) v\[?(\d+)(?::(\d+))?\]?,")


def test_nothing_writes_the_bias_operand_under_its_mfma(vsa, tmp_path):
    csrc = os.path.join(ROOT, "video-summarization_amd", "csrc")
    out = str(tmp_path / "vs_attention.s")
    r = subprocess.run([vsa._lib.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I" + csrc,
                        "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                        os.path.join(csrc, "vs_attention.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(out).read()
    kernels = list(re.finditer(r"^(_Z\w*attn_fwd_pipeI\w+):", text, re.M))
    assert len(kernels) >= 12
    for m in kernels:
        body = text[m.end():]
        body = body[:body.index(".Lfunc_end")]
        lines = [l.strip() for l in body.split("\n")]
        lines = [l if l.startswith(";;#ASM") else l.split(";")[0].strip() for l in lines]
        lines = [l for l in lines if l]
        sites = 0
        for i, l in enumerate(lines):
            if not (l.startswith("v_mfma") and lines[i - 1].startswith(";;#ASMSTART")):
                continue
            sites += 1
            c = re.match(r"v_mfma\S+ v\[\d+:\d+\], v\d+, v\d+, v\[(\d+):(\d+)\]", l)
            assert c, l
            c0, c1 = int(c.group(1)), int(c.group(2))
            for x in lines[i + 2:]:
                assert not (x.endswith(":") or x.startswith("s_cbranch") or x.startswith("s_branch")), (m.group(1), l, x)
                if x.startswith("v_mfma"):
                    break
                w = WRITES.match(x)
                if w and not x.startswith("v_cmp"):
                    a = int(w.group(2))
                    b = int(w.group(3) or a)
                    assert b < c0 or a > c1, (m.group(1), l, x)
        assert sites >= 3, (m.group(1), sites)          # loop body, remainder and last tile each start blocks this way
