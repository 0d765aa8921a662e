#!/usr/bin/env python3
"""Shift-invariant search of the code database (csrc/code_shift_search.hip) at NSynth's size: N = 305 979 stored sounds,
K = 512, synthetic uniform codes.  Cases: top maps F = 16, T = 64 with a window of W = 16 columns at all 49 offsets, Q = 1
and Q = 8; bottom maps F = 32, T = 128, W = 32, step 2, 49 offsets, Q = 1.  Per case, on the same box, in the same run, the
two candidates alternating A B A B:
  ours       isi_code_shift_search_f32 + isi_code_shift_best_f32 (distances at every offset, then the best offset per item)
  emulation  what a user had before: S calls of isi_code_search_f32 on S pre-cropped copies [N, F W] of the database,
             one per offset (the crops are made before the clock starts and timed separately; the emulation's own
             best-offset step is not timed at all, which favours it)
Device events around `iters` repetitions, median and min..max of `rounds` rounds; the distances of the two are compared
BITWISE before anything is timed.  Look-ups = N F W S Q per call.  The acceptance bar of DESIGN.md section 6c: the max of
ours over the rounds below the min of the emulation.  Writes profiles/code_search_shift.json.

  python tools/bench_code_search_shift.py [--rounds 5] [--iters 5] [--items 305979] [--out profiles/code_search_shift.json]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
import torch  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402


def _note(msg):
    print(f"[bench_code_search_shift] {msg}", file=sys.stderr, flush=True)


def _timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def _summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "rounds": [round(x, 4) for x in v]}


def shift_case(dev, name, codes, table, W, step, count, Q, rounds, iters, seed):
    """codes int16 [N, F, T] on the device (uint16 bit patterns below 2^15)."""
    lib = _hip.lib()
    N, F, T = codes.shape
    K = table.shape[0]
    g = torch.Generator(device=dev).manual_seed(seed)
    query = torch.randint(0, K, (Q, F, W), generator=g, device=dev, dtype=torch.int16)
    weights = torch.rand(Q, F, W, generator=g, device=dev) * 2.0
    stream = C.c_void_p(_hip.stream_ptr(dev))
    dist = torch.empty(Q, count, N, dtype=torch.float32, device=dev)
    best = torch.empty(Q, N, dtype=torch.float32, device=dev)
    best_shift = torch.empty(Q, N, dtype=torch.int32, device=dev)
    need = lib.isi_code_shift_search_workspace_bytes(N, F, T, W, count, K, Q)
    workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)

    def ours():
        _hip.check(lib.isi_code_shift_search_f32(codes.data_ptr(), query.data_ptr(), weights.data_ptr(), table.data_ptr(),
                                                 dist.data_ptr(), N, F, T, W, 0, step, count, K, Q, 0, workspace.data_ptr(),
                                                 workspace.numel() * 4, stream), "isi_code_shift_search_f32")
        _hip.check(lib.isi_code_shift_best_f32(dist.data_ptr(), None, best.data_ptr(), best_shift.data_ptr(), N, count, Q,
                                               stream), "isi_code_shift_best_f32")

    cells = F * W
    crops = torch.empty(count, N, cells, dtype=torch.int16, device=dev)

    def crop():
        for s in range(count):
            crops[s].view(N, F, W).copy_(codes[:, :, s * step:s * step + W])

    em_dist = torch.empty(count, Q, N, dtype=torch.float32, device=dev)
    em_need = lib.isi_code_search_workspace_bytes(N, cells, K, Q)
    em_workspace = torch.empty(em_need // 4, dtype=torch.float32, device=dev)

    def emulation():
        for s in range(count):
            _hip.check(lib.isi_code_search_f32(crops[s].data_ptr(), query.data_ptr(), weights.data_ptr(), table.data_ptr(), None,
                                               em_dist[s].data_ptr(), N, cells, K, Q, 0, em_workspace.data_ptr(), em_need,
                                               stream), "isi_code_search_f32")

    crop()
    ours()
    emulation()
    torch.cuda.synchronize()
    same = torch.equal(dist.view(torch.int32), em_dist.permute(1, 0, 2).contiguous().view(torch.int32))
    assert same, "the shifted search and its emulation differ in some bit"
    want_best, want_shift = em_dist.min(0)
    assert torch.equal(best, want_best) and bool((dist.gather(1, best_shift.long()[:, None, :])[:, 0] == best).all())
    del want_best, want_shift
    _timed(ours, 2)
    _timed(emulation, 1)
    times = {"ours": [], "emulation": []}
    for _ in range(rounds):
        times["ours"].append(_timed(ours, iters))
        times["emulation"].append(_timed(emulation, iters))
    crop_ms = _timed(crop, 1)
    res = {"layer": name, "N": N, "F": F, "T": T, "W": W, "step": step, "S": count, "K": K, "Q": Q,
           "bitwise_equal_to_the_emulation": same, "workspace_bytes": int(need), "dist_MB": round(dist.numel() * 4 / 1e6, 1),
           "emulation_crops_MB": round(crops.numel() * 2 / 1e6, 1), "emulation_crop_ms_not_included": round(crop_ms, 3),
           **{k: _summary(v) for k, v in times.items()}}
    lookups = N * cells * count * Q
    res["lookups_per_call_G"] = round(lookups / 1e9, 3)
    res["ours_lookups_per_second_T"] = round(lookups / res["ours"]["median_ms"] / 1e9, 3)
    res["emulation_lookups_per_second_T"] = round(lookups / res["emulation"]["median_ms"] / 1e9, 3)
    res["emulation_over_ours_median"] = round(res["emulation"]["median_ms"] / res["ours"]["median_ms"], 2)
    res["emulation_min_over_ours_max"] = round(res["emulation"]["min_ms"] / res["ours"]["max_ms"], 2)
    res["ours_max_below_emulation_min"] = res["ours"]["max_ms"] < res["emulation"]["min_ms"]
    _note(f"{name} Q={Q}: ours {res['ours']['median_ms']:.3f} ms ({res['ours']['min_ms']:.3f}..{res['ours']['max_ms']:.3f}), "
          f"emulation {res['emulation']['median_ms']:.3f} ms ({res['emulation']['min_ms']:.3f}..{res['emulation']['max_ms']:.3f}), "
          f"{res['ours_lookups_per_second_T']} T look-ups/s, crop {crop_ms:.2f} ms")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--items", type=int, default=305979)
    ap.add_argument("--codes", type=int, default=512)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "code_search_shift.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    N, K = args.items, args.codes
    g = torch.Generator(device=dev).manual_seed(0)
    codebook = torch.randn(K, 64, generator=g, device=dev)
    table = torch.empty(K, K, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().isi_code_distance_table_f32(codebook.data_ptr(), table.data_ptr(), K, 64,
                                                      C.c_void_p(_hip.stream_ptr(dev))), "isi_code_distance_table_f32")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "unit": "ms per call (device events)",
           "method": f"synthetic uniform codes; the two candidates alternate A B A B ...: {args.rounds} rounds of {args.iters} "
                     "repetitions each of isi_code_shift_search_f32 + isi_code_shift_best_f32 and of S calls of "
                     "isi_code_search_f32 on pre-cropped copies (crops and the emulation's best-offset step not timed); "
                     "spread = min..max of a candidate's rounds; distances compared bitwise before timing", "cases": []}
    for name, F, T, W, step, queries in (("top", 16, 64, 16, 1, (1, 8)), ("bottom", 32, 128, 32, 2, (1,))):
        codes = torch.randint(0, K, (N, F, T), generator=g, device=dev, dtype=torch.int16)
        for Q in queries:
            res["cases"].append(shift_case(dev, name, codes, table, W, step, 49, Q, args.rounds, args.iters, 10 * Q + len(name)))
        del codes
        torch.cuda.empty_cache()
    res["all_cases_meet_the_bar"] = all(c["ours_max_below_emulation_min"] for c in res["cases"])
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
