#!/usr/bin/env python3
"""Sampled codes/s of N variations of one request, `sample_model(num_variations=N)` (one shared encoder memory), against the
repeated-batch call that served the request before (`batch_size=N`, inputs repeated N times: the default path, unchanged).
One JSON line and profiles/sampling_variations.json (or --out):
  - the baseline top prior ([32,32], self-conditional, d_model 512, 6 + 8 layers), full mask: 1024 codes per row;
  - the baseline bottom prior ([64,64] over a [32,32] top map) on the 128-token window of tools/bench_sampling_kv16.py,
fp32 and bf16 caches, N = 1 / 8 / 32 / 128, all sides alternated in one process on one device.  The repeated batch is timed
TWICE, before and after the variations call: the difference of its two medians is the run-to-run spread the comparison has to
clear ("spread").  Per row: codes/s of the whole call, codes/s of the native loop alone (device time of NativeSampler.run
between two events: no encoder, no prefill) and the bytes of memory_kv.  Random weights, temperature 1, top-p 0.8; median of 3
calls after one warm-up.  --sides repeat --calls 1 runs the repeated batch alone (for a kernel trace of that path)."""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "interactive-spectrogram-inpainting_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

from bench_sampling_kv16 import CLS, FULL, LOOP, _instrument  # noqa: E402


def _time(fn, n_codes, calls):
    fn(0)
    torch.cuda.synchronize()
    ts, loops = [], []
    for rep in range(calls):
        LOOP["events"].clear()
        t0 = time.perf_counter()
        fn(1 + rep)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        loops.append(sum(a.elapsed_time(b) for a, b in LOOP["events"]) * 1e-3)
    mid = len(ts) // 2
    return {"codes_per_s": round(n_codes / sorted(ts)[mid], 1), "loop_codes_per_s": round(n_codes / sorted(loops)[mid], 1),
            "memory_kv_bytes": LOOP["bytes"][1]}


def _compare(out, tag, n_codes, repeat, variations, sides, calls):
    row = {}
    if "repeat" in sides:
        row["repeat"] = _time(repeat, n_codes, calls)
    if "variations" in sides:
        row["variations"] = _time(variations, n_codes, calls)
    if "repeat" in sides and "variations" in sides:
        row["repeat_again"] = _time(repeat, n_codes, calls)
        for key in ("codes_per_s", "loop_codes_per_s"):
            a, b, v = row["repeat"][key], row["repeat_again"][key], row["variations"][key]
            row[f"spread_{key}"] = round(abs(a - b) / max(a, b), 4)
            row[f"speedup_{key}"] = round(v / max(a, b), 4)        # against the better of the two repeated-batch timings
    out["rows"][tag] = row
    print(tag, row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--formats", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--sides", nargs="+", default=["repeat", "variations"], choices=["repeat", "variations"])
    ap.add_argument("--priors", nargs="+", default=["top", "bottom"], choices=["top", "bottom"])
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sampling_variations.json"))
    args = ap.parse_args()
    import sample as S
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer, UpsamplingVQTransformer
    _instrument()
    dev = torch.device("cuda", 0)
    dtypes = {"f32": torch.float32, "bf16": torch.bfloat16}
    out = {"unit": "sampled codes/s",
           "timing": f"median of {args.calls} calls after one warm-up; loop = device time of the native loop alone; repeat = "
                     "batch_size=N with the inputs repeated (num_variations=None), timed before and after the variations call; "
                     "spread = |repeat - repeat_again| / max; speedup = variations / max(repeat, repeat_again)",
           "device": torch.cuda.get_device_name(0), "rows": {}}
    if "top" in args.priors:
        torch.manual_seed(2)
        top = SelfAttentiveVQTransformer(shape=[32, 32], condition_shape=[32, 32], self_conditional_model=True,
                                         add_mask_token_to_symbols=True, **FULL).to(dev).eval()
        for N in args.batches:
            for name in args.formats:
                kw = dict(class_conditioning=CLS, top_p_sampling_p=0.8, kv_cache_dtype=dtypes[name])
                repeat = lambda seed: S.sample_model(top, dev, N, [32, 32], 1.0, generator=torch.Generator().manual_seed(seed), **kw)
                variations = lambda seed: S.sample_model(top, dev, 1, [32, 32], 1.0, num_variations=N,
                                                         generator=torch.Generator().manual_seed(seed), **kw)
                _compare(out, f"top_N{N}_{name}", 1024 * N, repeat, variations, args.sides, args.calls)
        del top
        torch.cuda.empty_cache()
    if "bottom" in args.priors:
        torch.manual_seed(3)
        bottom = UpsamplingVQTransformer(shape=[64, 64], condition_shape=[32, 32], **FULL).to(dev).eval()
        mask = torch.zeros(1, 64, 64, dtype=torch.bool)
        mask[:, :, 60:62] = True
        g = torch.Generator().manual_seed(23)
        cond = torch.randint(0, 512, (1, 32, 32), generator=g)
        init = torch.randint(0, 512, (1, 64, 64), generator=g)
        for N in args.batches:
            condN, initN = cond.repeat(N, 1, 1), init.repeat(N, 1, 1)
            for name in args.formats:
                kw = dict(class_conditioning=CLS, mask=mask, top_p_sampling_p=0.8, kv_cache_dtype=dtypes[name])
                repeat = lambda seed: S.sample_model(bottom, dev, N, [64, 64], 1.0, condition=condN, initial_code=initN,
                                                     generator=torch.Generator().manual_seed(seed), **kw)
                variations = lambda seed: S.sample_model(bottom, dev, 1, [64, 64], 1.0, condition=cond, initial_code=init,
                                                         num_variations=N, generator=torch.Generator().manual_seed(seed), **kw)
                _compare(out, f"bottom_N{N}_{name}", 128 * N, repeat, variations, args.sides, args.calls)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
