#!/usr/bin/env python3
"""Output hashes of the exact-fp32 attention (attn_fwd_pipe), recorded on an MI355X at the commit BEFORE the kernel's tile
loop was rescheduled:

    python tests/golden/make_golden_attention_bits.py [OUT.json]

For every case of tests/attention_bits_cases.py: the sha256 of the output tensor's bytes, and the recording build's own
distance from the float64 reference.  The limit of a random-input case is test_hip_parity.py's 2e-5; the limit of a spiked
case is 5e-5 (the rescale-branch test's) where the recording build is inside it, otherwise twice the recording build's own
error.  The packed ragged call is hashed too (logits, hidden state, scores), with whether its scores equal the padded batch's
bit for bit on the recording build.  tests/test_hip_attention_fp32_bits.py asserts all of it.
"""
import importlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
pkg = importlib.import_module("video-summarization_amd")
import attention_bits_cases as abc  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    out = {"direct": {}, "packed": {}}
    for name in [c[0] for c in abc.DIRECT] + abc.SPIKED:
        spiked = name in abc.SPIKED
        q, k, v, mask, scale = abc.spiked_inputs(name) if spiked else abc.direct_inputs(pkg.synth, name)
        o = abc.run_direct(pkg, q, k, v, mask, scale, dev)
        assert abc.sha(abc.run_direct(pkg, q, k, v, mask, scale, dev)) == abc.sha(o), name
        err = (o.double() - abc.attn_ref(q, k, v, mask, scale)).abs().max().item()
        if spiked:
            limit = abc.LIMIT_RESCALE if err < abc.LIMIT_RESCALE else 2.0 * err
        else:
            limit = abc.LIMIT_RANDOM
        out["direct"][name] = {"sha256": abc.sha(o), "recorded_err": err, "limit": limit}
        print("%-14s err %.3e limit %.1e %s" % (name, err, limit, abc.sha(o)[:16]))
    m = abc.packed_model(pkg, dev)
    vids = abc.packed_videos(pkg.synth)
    lengths = abc.PACKED_LENGTHS
    x = torch.cat(vids).to(dev)
    with torch.no_grad():
        logits, hidden = m.forward_packed(x, lengths)
        sc = m.score_packed(x, lengths)
        T = max(lengths)
        xp = torch.full((len(vids), T, vids[0].shape[1]), pkg.synth.PAD_VALUE)
        for i, vv in enumerate(vids):
            xp[i, :vv.shape[0]] = vv
        pm = pkg.synth.padding_mask(xp)
        sp = m.score(xp.to(dev), pm.to(dev))
        alone = torch.cat([m.score(vv[None].to(dev))[0] for vv in vids])
    out["packed"] = {"logits": abc.sha(logits), "hidden": abc.sha(hidden), "scores": abc.sha(sc),
                     "scores_equal_padded_batch": bool(torch.equal(sp.cpu()[~pm], sc.cpu())),
                     "scores_equal_each_alone": bool(torch.equal(alone.cpu(), sc.cpu()))}
    print(out["packed"])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "attention_fp32_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
