#!/usr/bin/env python3
"""Sampled codes/s of KV-cached sampling without and with a logit bias (sample_model's allowed_codes / code_bias /
code_bias_map, isi_prior_code_bias), one JSON line and profiles/sampling_code_bias.json (or --out):
  - the baseline top prior ([32,32], self-conditional, d_model 512, 6 + 8 layers), full mask: 1024 codes per sequence;
  - the baseline bottom prior ([64,64] over a [32,32] top map) on a 128-token window at the END of the map (two frames, every
    frequency; the prefix is prefilled by one batched pass),
at B = 1 / 8 / 32 / 128.  Modes: `off` (the keywords left out), `palette` (allowed_codes: a random half of the classes, one
table row for every cell) and `map` (a 4-row table -- two palettes, a dense bias, zeros -- chosen per cell by a random
code_bias_map that also holds -1).  One measuring process per tree: its modes alternate call by call; per mode the median
of --reps calls after one warm-up, codes/s of the whole `sample_model` call and of the native loop alone (device time of
NativeSampler.run between two events), and the spread of the calls, (slowest - fastest) / median.
(a) off against the parent commit: with --parent-tree (a checkout of the parent, built there) the processes alternate
parent, this tree, parent, ... for --rounds rounds in one session; per row `off_over_parent` = ratio of the medians over the
rounds, beside each side's spread over its rounds -- the parent's is its own run-to-run spread, the yardstick for the ratio.
(b) `palette_over_off`, `map_over_off`: ratios of the medians over the rounds, modes alternating inside each process.
Random weights, temperature 1, top-p 0.8."""
import argparse
import json
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]

FULL = dict(n_class=512, channel=256, kernel_size=5, n_block=4, n_res_block=4, res_channel=256, d_model=512,
            embeddings_dim=32, positional_embeddings_dim=16, use_relative_transformer=True,
            predict_frequencies_first=True, conditional_model=True, class_conditioning_prepend_to_dummy_input=True,
            class_conditioning_num_classes_per_modality={"instrument_family_str": 11, "pitch": 61},
            class_conditioning_embedding_dim_per_modality={"instrument_family_str": 64, "pitch": 64})
LOOP = {"events": []}


def _instrument():
    """Device time of the native loop alone, read off NativeSampler.run."""
    import torch
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    orig = NativeSampler.run

    def run(self, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig(self, *a, **k)
        e1.record()
        LOOP["events"].append((e0, e1))

    NativeSampler.run = run


def _median(v):
    return sorted(v)[len(v) // 2]


def _spread(v):
    return round((max(v) - min(v)) / _median(v), 4)


def _time(fns, n_codes, reps):
    """fns: {mode: fn(seed)}; the modes alternate call by call.  Per mode: medians and spreads of the calls."""
    import torch
    for fn in fns.values():
        fn(0)
    torch.cuda.synchronize()
    ts = {m: [] for m in fns}
    loops = {m: [] for m in fns}
    for rep in range(reps):
        for m, fn in fns.items():
            LOOP["events"].clear()
            t0 = time.perf_counter()
            fn(1 + rep)
            torch.cuda.synchronize()
            ts[m].append(time.perf_counter() - t0)
            loops[m].append(sum(a.elapsed_time(b) for a, b in LOOP["events"]) * 1e-3)
    return {m: {"codes_per_s": round(n_codes / _median(ts[m]), 1), "spread": _spread(ts[m]),
                "loop_codes_per_s": round(n_codes / _median(loops[m]), 1), "loop_spread": _spread(loops[m])} for m in fns}


def _bias_modes(model, off_only):
    """{mode: sample_model keywords}"""
    import torch
    if off_only:
        return {"off": {}}
    n, (F, T) = model.n_class_target, model.shape
    g = torch.Generator().manual_seed(31)
    half = torch.zeros(n, dtype=torch.bool)
    half[torch.randperm(512, generator=g)[:256]] = True
    table = torch.zeros(4, n)
    table[0, ~half] = -float("inf")
    table[1, half] = -float("inf")
    table[2] = 3.0 * torch.randn(n, generator=g)
    cells = torch.randint(-1, 4, (F, T), generator=g)
    return {"off": {}, "palette": {"allowed_codes": half}, "map": {"code_bias": table, "code_bias_map": cells}}


def measure(args):
    """One tree, in this process: {row: {mode: figures}}."""
    tree = pathlib.Path(args.tree).resolve()
    for p in (str(tree), str(tree / "interactive-spectrogram-inpainting_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import sample as S
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer, UpsamplingVQTransformer
    _instrument()
    dev = torch.device("cuda", 0)
    cls = {"pitch": torch.tensor([24]), "instrument_family_str": torch.tensor([0])}
    rows = {}
    torch.manual_seed(2)
    top = SelfAttentiveVQTransformer(shape=[32, 32], condition_shape=[32, 32], self_conditional_model=True,
                                     add_mask_token_to_symbols=True, **FULL).to(dev).eval()
    modes = _bias_modes(top, args.off_only)
    for B in args.batches:
        fns = {name: (lambda seed, kw=kw: S.sample_model(top, dev, B, [32, 32], 1.0, class_conditioning=cls,
                                                         top_p_sampling_p=0.8,
                                                         generator=torch.Generator().manual_seed(seed), **kw))
               for name, kw in modes.items()}
        rows[f"top_B{B}"] = _time(fns, 1024 * B, args.reps)
        print(f"top_B{B}", rows[f"top_B{B}"], file=sys.stderr, flush=True)
    del top
    torch.cuda.empty_cache()
    torch.manual_seed(3)
    bottom = UpsamplingVQTransformer(shape=[64, 64], condition_shape=[32, 32], **FULL).to(dev).eval()
    modes = _bias_modes(bottom, args.off_only)
    mask = torch.zeros(1, 64, 64, dtype=torch.bool)
    mask[:, :, 60:62] = True
    for B in args.batches:
        g = torch.Generator().manual_seed(23)
        cond = torch.randint(0, 512, (B, 32, 32), generator=g)
        init = torch.randint(0, 512, (B, 64, 64), generator=g)
        fns = {name: (lambda seed, kw=kw: S.sample_model(bottom, dev, B, [64, 64], 1.0, condition=cond,
                                                         class_conditioning=cls, initial_code=init, mask=mask,
                                                         top_p_sampling_p=0.8,
                                                         generator=torch.Generator().manual_seed(seed), **kw))
               for name, kw in modes.items()}
        rows[f"bottom_B{B}"] = _time(fns, 128 * B, args.reps)
        print(f"bottom_B{B}", rows[f"bottom_B{B}"], file=sys.stderr, flush=True)
    return {"device": torch.cuda.get_device_name(0), "rows": rows}


def _child(args, tree, off_only):
    """A fresh measuring process for one tree (this script, that tree's package and library)."""
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--measure", "--tree", str(tree), "--reps", str(args.reps),
           "--batches", *map(str, args.batches)] + (["--off-only"] if off_only else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=args.child_timeout)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true", help="measure --tree in this process and print its figures")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--tree", default=str(ROOT), help="checkout of the project to measure (default: this one)")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: measured alternately with this tree")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child-timeout", type=float, default=900.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sampling_code_bias.json"))
    args = ap.parse_args()
    if args.measure:
        print(json.dumps(measure(args)))
        return
    runs = {"parent": [], "this": []}
    for rnd in range(args.rounds):
        if args.parent_tree:
            runs["parent"].append(_child(args, args.parent_tree, True))
        runs["this"].append(_child(args, args.tree, args.off_only))
        print(f"round {rnd + 1} of {args.rounds} done", file=sys.stderr, flush=True)
    out = {"unit": "sampled codes/s",
           "timing": f"{args.rounds} rounds, one process per tree and round, parent and this tree alternating; in a process the "
                     f"median of {args.reps} calls after one warm-up, modes alternating call by call; figures below: median "
                     "over the rounds, rounds_spread = (largest - smallest) / median over the rounds, calls_spread = the "
                     "largest spread of the calls inside a round; loop = device time of the native loop alone",
           "device": runs["this"][0]["device"], "rows": {}}
    for key in runs["this"][0]["rows"]:
        row = {}
        sides = [("parent_off", runs["parent"], "off")] if args.parent_tree else []
        sides += [(m, runs["this"], m) for m in runs["this"][0]["rows"][key]]
        for name, side, mode in sides:
            for fig, sp in (("codes_per_s", "spread"), ("loop_codes_per_s", "loop_spread")):
                v = [r["rows"][key][mode][fig] for r in side]
                row.setdefault(name, {}).update({fig: _median(v), f"{fig}_rounds_spread": _spread(v),
                                                 f"{fig}_calls_spread": max(r["rows"][key][mode][sp] for r in side)})
        for num, den in (("off", "parent_off"), ("palette", "off"), ("map", "off")):
            if num in row and den in row:
                tag = "off_over_parent" if den == "parent_off" else f"{num}_over_off"
                row[tag] = round(row[num]["codes_per_s"] / row[den]["codes_per_s"], 4)
                row["loop_" + tag] = round(row[num]["loop_codes_per_s"] / row[den]["loop_codes_per_s"], 4)
        out["rows"][key] = row
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
