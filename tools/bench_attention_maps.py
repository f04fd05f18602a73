#!/usr/bin/env python3
"""Attention maps on request: what they cost beside the forward they ride on (device events after warm-up, the legs
alternating inside one process).

    python tools/bench_attention_maps.py [--reps 7] [--json profiles/attention_maps_bench.json] [--skip-long]

Shapes (M-A: 4 heads, d_model 256, 4 layers): one T = 320 video; B = 64, T = 1024; 8 videos of T = 8192 with 2048-d features.
Legs: `forward`, `attention_summary`, `attention_maps` and - context only - a torch-ops restatement of the maps on the same
GPU (the reference's arithmetic, every layer's softmax kept).  The long shape runs the first two only: its maps would be
8.6 GB per layer.  Yardsticks, taken in the same run from code that does not depend on the new kernels:
  * (attention_summary - forward) per layer against the attention stage of the forward (vs_profile_collect): the two new
    passes do two T^2 dh products per head, the MFMA count of the attention forward they sit beside;
  * (attention_maps - attention_summary) against the bytes of the maps over 6.29 TB/s, the achievable HBM rate of
    MI355X_MICROARCH.md (the stores overlap the products of the same kernel: this difference is what the maps ADD, not a
    bandwidth measurement).

    python tools/bench_attention_maps.py --packed [--seed 7] [--out profiles/attention_maps_packed_bench.txt]

The packed leg: a ragged batch - 64 videos of `synth.corpus_lengths(64, seed)` (100 to 650 frames) and the reference's B = 4 -
through `attention_summary_packed` / `attention_maps_packed` against `attention_summary` / `attention_maps` on the same videos
right-padded to the longest with the 1000.0 sentinel and the key mask; `forward_packed` and `forward` beside them, because the
forward inside the call does not shrink by the side kernels' factor.  All legs alternate inside this one process.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

vsa = importlib.import_module("video-summarization_amd")
HBM_ACHIEVABLE_TBS = 6.29
H, D, L = 4, 256, 4


def torch_maps(params, x, mask):
    """logits and every layer's softmax weights in torch ops (reference simnet.py:148-164 in eval mode)"""
    B, T, _ = x.shape
    dh = D // H
    h = F.linear(x, params["embedding_layer.feature_transform.weight"], params["embedding_layer.feature_transform.bias"])
    h = h + params["embedding_layer.positional_encoding.pos_embedding"][:, :T]
    maps = []
    for l in range(L):
        pre = "encoder.module_list.%d." % l
        lin = lambda t, n: F.linear(t, params[pre + n + ".weight"], params[pre + n + ".bias"])     # noqa: E731
        q = lin(h, "sa.q").view(B, T, H, dh).permute(0, 2, 1, 3)
        k = lin(h, "sa.k").view(B, T, H, dh).permute(0, 2, 1, 3)
        v = lin(h, "sa.v").view(B, T, H, dh).permute(0, 2, 1, 3)
        s = torch.matmul(q, k.transpose(2, 3)) * D ** -0.5
        if mask is not None:
            s = s.masked_fill(mask.view(B, 1, 1, T), float("-inf"))
        w = F.softmax(s, dim=3)
        maps.append(w)
        o = lin(torch.matmul(w, v).permute(0, 2, 1, 3).contiguous().view(B, T, D), "sa.feature_projection")
        h = F.layer_norm(o + h, (D,), params[pre + "norm1.weight"], params[pre + "norm1.bias"], 1e-5)
        f = lin(F.relu(lin(h, "mlp.fc1")), "mlp.fc2")
        h = F.layer_norm(f + h, (D,), params[pre + "norm2.weight"], params[pre + "norm2.bias"], 1e-5)
    return F.linear(h, params["final_layer.weight"], params["final_layer.bias"]), maps


def time_legs(legs, reps):
    """{name: median ms}: every leg warmed up, then `reps` rounds that run the legs one after the other"""
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in legs}
    for _ in range(reps):
        for n, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[n].append(a.elapsed_time(b))
    return {n: float(np.median(v)) for n, v in ts.items()}, {n: float(np.min(v)) for n, v in ts.items()}


def attention_stage_ms(model, x, reps):
    """the forward's attention stage, all layers, per call (HIP events around the stage inside the library)"""
    lib = vsa._lib.load()
    with torch.no_grad():
        model(x)
        torch.cuda.synchronize()
        lib.vs_profile_enable(1)
        for _ in range(reps):
            model(x)
        torch.cuda.synchronize()
        ms, n = vsa._lib.profile_collect()["attention"]
        lib.vs_profile_enable(0)
    return ms / reps, n // reps


def time_legs_spread(legs, reps):
    """{name: (median, min, max) ms}: time_legs' loop, keeping the spread"""
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in legs}
    for _ in range(reps):
        for n, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[n].append(a.elapsed_time(b))
    return {n: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for n, v in ts.items()}


def packed_legs(args, dev):
    """packed against padded on the same ragged videos; returns the lines of the report"""
    sd = vsa.synth.make_state_dict(D, L, 3)
    model = vsa.SimNet(num_heads=H, d_model=D, num_layers=L, sparsity=0.0, dropout=0.3)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    lines = []
    for B in (64, 4):
        lengths = vsa.synth.corpus_lengths(B, args.seed)
        tmax, M = max(lengths), sum(lengths)
        x = vsa.synth.make_features(B, tmax, 4, "randn", lengths).to(dev)          # right-padded with the sentinel
        mask = vsa.synth.padding_mask(x)
        xp = torch.cat([x[b, :t] for b, t in enumerate(lengths)], dim=0).contiguous()

        def fwd():
            with torch.no_grad():
                return model(x, mask)

        legs = {"forward padded": fwd, "forward packed": lambda: model.forward_packed(xp, lengths, want_hidden=False),
                "summary padded": lambda: model.attention_summary(x, mask),
                "summary packed": lambda: model.attention_summary_packed(xp, lengths),
                "maps padded": lambda: model.attention_maps(x, mask), "maps packed": lambda: model.attention_maps_packed(xp, lengths)}
        t = time_legs_spread(legs, args.reps)
        sq = sum(u * u for u in lengths)
        lines.append("B=%-3d lengths %d..%d (seed %d)   rows %d packed / %d padded   fill %.3f   sum T^2 / (B Tmax^2) %.3f"
                     % (B, min(lengths), tmax, args.seed, M, B * tmax, M / (B * tmax), sq / (B * tmax * tmax)))
        for what in ("forward", "summary", "maps"):
            (pm, plo, phi), (km, klo, khi) = t[what + " padded"], t[what + " packed"]
            lines.append("  %-8s padded %7.3f ms (%.3f..%.3f)   packed %7.3f ms (%.3f..%.3f)   packed / padded %.3f"
                         % (what, pm, plo, phi, km, klo, khi, km / pm))
        side_pad = t["summary padded"][0] - t["forward padded"][0]
        side_pk = t["summary packed"][0] - t["forward packed"][0]
        lines.append("  summary - forward (the side kernels, %d layers): padded %.3f ms, packed %.3f ms (%.3f)"
                     % (L, side_pad, side_pk, side_pk / side_pad if side_pad > 0 else float("nan")))
        lines.append("  map memory, all %d layers: padded %.1f MiB, packed %.1f MiB (%.3f)"
                     % (L, L * B * H * tmax * tmax * 4 / 2 ** 20, L * H * sq * 4 / 2 ** 20, sq / (B * tmax * tmax)))
        lines.append("")
        print("\n".join(lines[-7:]), flush=True)
        del x, xp, mask
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--packed", action="store_true", help="run the packed-against-padded legs only")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_maps_packed_bench.txt"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "attention_maps_bench.json"))
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda", 0)
    if args.packed:
        head = ["Attention maps and summaries on packed ragged batches against the padded calls - measured on one MI355X",
                "=" * 103, "",
                "tools/bench_attention_maps.py --packed --reps %d --seed %d; model M-A (H%d / d%d / L%d), every layer selected, exact fp32."
                % (args.reps, args.seed, H, D, L),
                "Device events around each call after two warm-up calls per leg; the six legs alternate inside one process, %d rounds:" % args.reps,
                "median (min..max).  Lengths: synth.corpus_lengths(B, seed), uniform 100..650 frames; the padded legs take the same videos",
                "right-padded to the longest with the 1000.0 sentinel and the key mask.  sum T^2 / (B Tmax^2) is the ratio of the side",
                "kernels' work and of the map memory; the forward inside each call does not shrink by that factor.", ""]
        lines = head + packed_legs(args, dev)
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines))
        return
    shapes = [dict(name="b1_t320", B=1, T=320, fin=1024, pe=2000, maps=True),
              dict(name="b64_t1024", B=64, T=1024, fin=1024, pe=2000, maps=True)]
    if not args.skip_long:
        shapes.append(dict(name="b8_t8192_f2048", B=8, T=8192, fin=2048, pe=8192, maps=False))
    rows = []
    for s in shapes:
        sd = vsa.synth.make_state_dict(D, L, 3, in_features=s["fin"], max_len=s["pe"])
        model = vsa.SimNet(num_heads=H, d_model=D, num_layers=L, sparsity=0.0, dropout=0.3, in_features=s["fin"], pe_len=s["pe"])
        model.load_state_dict(sd, strict=True)
        model = model.to(dev).eval()
        x = vsa.synth.make_features(s["B"], s["T"], 4, "randn", in_features=s["fin"]).to(dev)
        params = {k: v.to(dev) for k, v in sd.items()}

        def fwd():
            with torch.no_grad():
                return model(x)

        legs = {"forward": fwd, "attention_summary": lambda: model.attention_summary(x)}
        if s["maps"]:
            legs["attention_maps"] = lambda: model.attention_maps(x)

            def tmaps():
                with torch.no_grad():
                    return torch_maps(params, x, None)
            legs["torch_ops_maps"] = tmaps
        med, best = time_legs(legs, args.reps)
        att_ms, att_launches = attention_stage_ms(model, x, args.reps)
        row = dict(shape=s["name"], B=s["B"], T=s["T"], layers=L, reps=args.reps,
                   ms_median={k: round(v, 4) for k, v in med.items()}, ms_min={k: round(v, 4) for k, v in best.items()},
                   attention_stage_ms_per_layer=round(att_ms / L, 4), attention_stage_launches=att_launches,
                   summary_extra_ms_per_layer=round((med["attention_summary"] - med["forward"]) / L, 4))
        row["summary_extra_over_attention_stage"] = round(row["summary_extra_ms_per_layer"] / row["attention_stage_ms_per_layer"], 2)
        if s["maps"]:
            nbytes = L * s["B"] * H * s["T"] * s["T"] * 4
            extra = med["attention_maps"] - med["attention_summary"]
            floor = nbytes / (HBM_ACHIEVABLE_TBS * 1e12) * 1e3
            # the stores run under the MFMAs of the same kernel, so the difference can come out BELOW the pure-store floor;
            # the rate of the storing kernel itself is in the kernel trace (profiles/attention_maps_kernel_stats.txt)
            row.update(maps_bytes=nbytes, maps_extra_ms=round(extra, 4), maps_store_floor_ms=round(floor, 4),
                       maps_extra_over_store_floor=round(extra / floor, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del model, x, params
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
