#!/usr/bin/env python3
"""Sampled codes/s of KV-cached sampling without and with per-token log-probabilities (return_log_probs), one JSON line and
profiles/sampling_logprobs.json (or --out):
  - the baseline top prior ([32,32], self-conditional, d_model 512, 6 + 8 layers), full mask: 1024 codes per sequence;
  - the baseline bottom prior ([64,64] over a [32,32] top map) on a 128-token window at the END of the map (two frames, every
    frequency: positions 3840 .. 3967; the prefix is prefilled by one batched pass),
at B = 1 / 8 / 32 / 128, the option off and on alternated call by call in the same process on the same device.  Per row:
codes/s of the whole `sample_model` call and of the native loop alone (device time of NativeSampler.run between two events:
no encoder, no prefill) -- the median of --reps calls after one warm-up -- and the spread of the calls,
(slowest - fastest) / median.  Random weights, temperature 1, top-p 0.8.  `on_over_off` = ratio of the medians.
--off-only leaves the keyword out altogether; with --tree it measures another checkout of the project (the parent commit,
built there) with this script, for the off path's run-to-run comparison."""
import argparse
import json
import pathlib
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
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: round((max(v) - min(v)) / med(v), 4)
    return {m: {"codes_per_s": round(n_codes / med(ts[m]), 1), "spread": spread(ts[m]),
                "loop_codes_per_s": round(n_codes / med(loops[m]), 1), "loop_spread": spread(loops[m])} for m in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--tree", default=str(ROOT), help="checkout of the project to measure (default: this one)")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sampling_logprobs.json"))
    args = ap.parse_args()
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
    modes = [("off", {})] if args.off_only else [("off", {}), ("on", {"return_log_probs": True})]
    out = {"unit": "sampled codes/s",
           "timing": f"median of {args.reps} calls after one warm-up, modes alternating call by call; spread = (slowest - "
                     "fastest) / median; loop = device time of the native loop alone",
           "device": torch.cuda.get_device_name(0), "rows": {}}

    def record(key, res):
        if "on" in res:
            res["on_over_off"] = round(res["on"]["codes_per_s"] / res["off"]["codes_per_s"], 4)
            res["loop_on_over_off"] = round(res["on"]["loop_codes_per_s"] / res["off"]["loop_codes_per_s"], 4)
        out["rows"][key] = res
        print(key, res, flush=True)

    torch.manual_seed(2)
    top = SelfAttentiveVQTransformer(shape=[32, 32], condition_shape=[32, 32], self_conditional_model=True,
                                     add_mask_token_to_symbols=True, **FULL).to(dev).eval()
    for B in args.batches:
        fns = {name: (lambda seed, kw=kw: S.sample_model(top, dev, B, [32, 32], 1.0, class_conditioning=cls,
                                                         top_p_sampling_p=0.8,
                                                         generator=torch.Generator().manual_seed(seed), **kw))
               for name, kw in modes}
        record(f"top_B{B}", _time(fns, 1024 * B, args.reps))
    del top
    torch.cuda.empty_cache()
    torch.manual_seed(3)
    bottom = UpsamplingVQTransformer(shape=[64, 64], condition_shape=[32, 32], **FULL).to(dev).eval()
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
               for name, kw in modes}
        record(f"bottom_B{B}", _time(fns, 128 * B, args.reps))
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
