#!/usr/bin/env python3
"""Rows/s of the row-statistics kernel beside the log-probability kernel, one JSON line and profiles/token_stats.json (or --out).

Over the same random logit rows, alternating launch batch by launch batch in one process: `isi_token_log_prob_f32` alone and
`isi_token_stats_f32` (all outputs) with top_n = 0, 4 and 16, at
  - top:    32 x 1024 rows of the baseline top prior's class count,
  - bottom:  8 x 4100 rows of the baseline bottom prior's.
Per entry: the median over --reps batches of (device time between two events around --iters launches) / iters, after one
warm-up batch; rows/s; bytes of logits read per second (rows x n x 4 bytes over that time: the bytes the algorithm needs,
not a memory-counter reading -- at these sizes the rows fit the last-level cache); spread = (slowest - fastest) / median.
`stats0_over_log_prob` is the ratio of the two median times.  Both kernels read the same bytes from memory; the
log-probability kernel walks the row twice (maximum, sum), the statistics kernel at top_n = 0 three times (maximum, sum with
the entropy term, rank) with one more barrier and two more stores, so about 1.5 is expected (measured on the MI355X: 1.43 - 1.44) and the ratio is CHECKED against
STATS0_FACTOR = 3: beyond it the record says `"stats0_within_factor": false` and the script exits with status 1.

--parent-sample PATH: the parent commit's sample.py.  It is loaded beside this tree's in the same process, over the same
package and library, and `score_codemap` of both is timed call by call in turn on the baseline top prior (B = 8) and bottom
prior (B = 2) -- what the refactor of its preamble costs -- and the two results are compared bit for bit.  CHECKED (exit
status 1 otherwise): the results are bit-identical and `this_over_parent` is at most 1 + the larger of the two spreads
(`within_spread`).  Without it that part is reported as not measured."""
import argparse
import importlib.util
import json
import pathlib
import sys
import time

STATS0_FACTOR = 3.0

ROOT = pathlib.Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "interactive-spectrogram-inpainting_amd"), str(ROOT / "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _median(v):
    return sorted(v)[len(v) // 2]


def _spread(v):
    return round((max(v) - min(v)) / _median(v), 4)


def time_kernels(name, rows, n, iters, reps):
    import torch
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.priors import _ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(rows + n)
    logits = (torch.randn(rows, n, generator=g) * 3).to(dev)
    codes = torch.randint(0, n, (rows,), generator=g).to(dev)
    # the C entries themselves, outputs allocated once: no allocation and no wrapper between two launches
    L, stream = _hip.lib(), torch.cuda.current_stream().cuda_stream
    lp = torch.empty(rows, dtype=torch.float32, device=dev)
    st_lp, ent = torch.empty_like(lp), torch.empty_like(lp)
    rank = torch.empty(rows, dtype=torch.int32, device=dev)
    top_codes = torch.empty(rows, 16, dtype=torch.int64, device=dev)
    top_lp = torch.empty(rows, 16, dtype=torch.float32, device=dev)
    fns = {"log_prob": lambda: L.isi_token_log_prob_f32(logits.data_ptr(), n, rows, n, codes.data_ptr(), lp.data_ptr(), stream)}
    for top_n in (0, 4, 16):
        fns[f"stats_top{top_n}"] = (lambda top_n=top_n: L.isi_token_stats_f32(
            logits.data_ptr(), n, rows, n, codes.data_ptr(), st_lp.data_ptr(), ent.data_ptr(), rank.data_ptr(), top_n,
            top_codes.data_ptr(), top_lp.data_ptr(), stream))
    for k, fn in fns.items():
        _hip.check(fn(), k)
    torch.cuda.synchronize()
    assert torch.equal(st_lp, lp) and torch.equal(lp, _ops.token_log_probs(logits, codes)), "the two kernels disagree"
    ms = {k: [] for k in fns}
    for rep in range(reps + 1):                                  # batch 0 warms up
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms[k].append(e0.elapsed_time(e1) / iters)
    res = {"rows": rows, "n_class": n, "logit_bytes": rows * n * 4}
    for k, v in ms.items():
        t = _median(v) * 1e-3
        res[k] = {"us_per_call": round(t * 1e6, 2), "rows_per_s": round(rows / t, 1),
                  "logit_bytes_per_s": round(rows * n * 4 / t, 1), "spread": _spread(v)}
    res["stats0_over_log_prob"] = round(res["stats_top0"]["us_per_call"] / res["log_prob"]["us_per_call"], 3)
    res["stats0_within_factor"] = res["stats0_over_log_prob"] <= STATS0_FACTOR
    print(name, res, flush=True)
    return res


def time_score_codemap(parent_path, top, bottom, reps):
    import torch
    import sample as S
    spec = importlib.util.spec_from_file_location("parent_sample", parent_path)
    parent = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(parent)
    dev = torch.device("cuda", 0)
    cls = {"pitch": torch.tensor([24]), "instrument_family_str": torch.tensor([0])}
    out = {}
    g = torch.Generator().manual_seed(5)
    cases = {"top_B8": (top, torch.randint(0, 512, (8, 32, 32), generator=g), None),
             "bottom_B2": (bottom, torch.randint(0, 512, (2, 64, 64), generator=g), torch.randint(0, 512, (2, 32, 32), generator=g))}
    for name, (model, codemap, cond) in cases.items():
        mask = torch.zeros(1, *model.shape, dtype=torch.bool)
        mask[:, :, 8:24] = True
        fns = {"parent": lambda: parent.score_codemap(model, dev, codemap, condition=cond, class_conditioning=cls, mask=mask),
               "this": lambda: S.score_codemap(model, dev, codemap, condition=cond, class_conditioning=cls, mask=mask)}
        same = bool(torch.equal(fns["parent"](), fns["this"]()))
        ts = {k: [] for k in fns}
        for rep in range(reps + 1):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    ts[k].append(time.perf_counter() - t0)
        out[name] = {k: {"ms_per_call": round(_median(v) * 1e3, 3), "spread": _spread(v)} for k, v in ts.items()}
        out[name]["this_over_parent"] = round(_median(ts["this"]) / _median(ts["parent"]), 4)
        out[name]["bit_identical"] = same
        out[name]["within_spread"] = out[name]["this_over_parent"] <= 1 + max(out[name][k]["spread"] for k in fns)
        print(name, out[name], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-sample", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "token_stats.json"))
    args = ap.parse_args()
    import torch
    from bench_sampling_logprobs import FULL
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer, UpsamplingVQTransformer
    assert torch.cuda.is_available(), "bench_token_stats.py measures on the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(2)
    top = SelfAttentiveVQTransformer(shape=[32, 32], condition_shape=[32, 32], self_conditional_model=True,
                                     add_mask_token_to_symbols=True, **FULL).to(dev).eval()
    torch.manual_seed(3)
    bottom = UpsamplingVQTransformer(shape=[64, 64], condition_shape=[32, 32], **FULL).to(dev).eval()
    out = {"timing": f"median of {args.reps} batches of {args.iters} launches between two device events after one warm-up "
                     "batch, entries alternating batch by batch; spread = (slowest - fastest) / median",
           "device": torch.cuda.get_device_name(0), "stats0_factor": STATS0_FACTOR, "kernels": {}}
    out["kernels"]["top_32x1024"] = time_kernels("top_32x1024", 32 * 1024, int(top.n_class_target), args.iters, args.reps)
    out["kernels"]["bottom_8x4100"] = time_kernels("bottom_8x4100", 8 * 4100, int(bottom.n_class_target), args.iters, args.reps)
    if args.parent_sample:
        out["score_codemap"] = time_score_codemap(args.parent_sample, top, bottom, args.reps)
    else:
        out["score_codemap"] = "not measured (no --parent-sample)"
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    failed = [k for k, v in out["kernels"].items() if not v["stats0_within_factor"]]
    if args.parent_sample:
        failed += [k for k, v in out["score_codemap"].items() if not (v["bit_identical"] and v["within_spread"])]
    if failed:
        sys.exit(f"bench_token_stats: expectation missed at {failed}")


if __name__ == "__main__":
    main()
