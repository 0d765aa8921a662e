#!/usr/bin/env python3
"""Search of the code database by encoder vectors at NSynth's size: N = 305 979 stored sounds,
K = 512 codes of D = 64 dimensions, synthetic uniform codes; top maps (F = 16, T = 64: 1024 cells) and bottom maps (F = 32,
T = 128: 4096 cells), Q = 1 and Q = 8 queries.  Per case, in ONE run, after a warm-up, the candidates alternating
A B C ... A B C ...:
  rows            isi_code_query_rows_f32: the Q queries' vectors [Q * C, 64] -> rows [Q, C, 512]
  torch_rows      the torch expression of the same rows, cdist(z, E) ** 2, followed by the gather a torch search needs
                  (rows.gather over one stored item's codes -- the smallest search there is) -- what a user had before
  hard            isi_code_search_f32            (query codes + the [K, K] table)
  soft            isi_code_search_rows_f32       (the rows, built before the clock starts)
  hard_again      isi_code_search_f32 once more: two identical candidates, whose difference is the run-to-run spread
  hard_parent     isi_code_search_f32 of the PARENT commit's library (--parent-lib), to show the hard search did not move
and for the 49-offset window search (top maps W = 16; bottom maps W = 32, step 2), at Q = 1 and Q = 8 on both:
  shift_hard / shift_soft / shift_hard_again / shift_hard_parent   the same four for isi_code_shift_search_(rows_)f32
Device events around `iters` repetitions, median and min..max of `rounds` rounds.  The tool REFUSES to time a case unless
the rows search on rows gathered from the table, rows[j][c] = T[query[j][c]], matches the hard search bit for bit at that
size (contracts 2 and 3), and unless the parent's library gives the hard search's bits.  There is no pass or fail bar on the
soft search's time; soft / hard is reported.  The hard searches are meant to be unchanged: where the parent library's median
lies outside the min..max of the two identical runs of a case, the tool says so loudly, still writes the record, and exits
with status 3.  Writes profiles/code_search_soft.json.

  python tools/bench_code_search_soft.py [--parent-lib PATH] [--rounds 5] [--iters 5] [--items 305979] [--out ...]
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

D = 64
HARD_SYMBOLS = ("isi_code_search_f32", "isi_code_shift_search_f32", "isi_code_search_workspace_bytes",
                "isi_code_shift_search_workspace_bytes", "isi_last_error")


def _note(msg):
    print(f"[bench_code_search_soft] {msg}", file=sys.stderr, flush=True)


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


def _parent(path):
    """The parent commit's library, loaded beside this one, with the hard searches' signatures."""
    if path is None:
        return None
    handle = C.CDLL(str(pathlib.Path(path).resolve()))
    for name in HARD_SYMBOLS:
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _hip.SIGNATURES[name]
    return handle


def _alternate(candidates, rounds, iters):
    for fn in candidates.values():                                    # warm-up: every candidate, twice
        _timed(fn, 2)
    times = {name: [] for name in candidates}
    for _ in range(rounds):
        for name, fn in candidates.items():
            times[name].append(_timed(fn, iters))
    return {name: _summary(v) for name, v in times.items()}


def _ratios(res, hard, soft, again, parent):
    h = res[hard]["median_ms"]
    res["soft_over_hard_median"] = round(res[soft]["median_ms"] / h, 3)
    spread = abs(res[again]["median_ms"] - h) / h
    lo = min(res[hard]["min_ms"], res[again]["min_ms"])
    hi = max(res[hard]["max_ms"], res[again]["max_ms"])
    res["identical_runs_median_difference"] = round(spread, 4)
    res["identical_runs_min_max_ms"] = [lo, hi]
    if parent in res:
        res["hard_over_parent_median"] = round(h / res[parent]["median_ms"], 4)
        res["parent_median_inside_identical_runs_min_max"] = bool(lo <= res[parent]["median_ms"] <= hi)


def case(dev, parent, name, codes, table, codebook, Q, rounds, iters, seed, W, step, count):
    """codes int16 [N, F, T] on the device (uint16 bit patterns below 2^15)."""
    lib = _hip.lib()
    N, F, T = codes.shape
    K, cells = table.shape[0], F * T
    g = torch.Generator(device=dev).manual_seed(seed)
    stream = C.c_void_p(_hip.stream_ptr(dev))
    query = torch.randint(0, K, (Q, F, T), generator=g, device=dev, dtype=torch.int16)
    weights = torch.rand(Q, F, T, generator=g, device=dev) * 2.0
    z = codebook[query.long()] + 0.5 * torch.randn(Q, F, T, D, generator=g, device=dev)       # noisy code vectors
    rows = torch.empty(Q, cells, K, dtype=torch.float32, device=dev)
    gathered = table[query.reshape(Q, cells).long()].contiguous()                           # contract 2's rows
    dist = {k: torch.empty(Q, N, dtype=torch.float32, device=dev) for k in ("hard", "soft", "parent")}
    need = lib.isi_code_search_workspace_bytes(N, cells, K, Q)
    workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
    one_item = codes[:1].reshape(1, cells).long()

    def build():
        _hip.check(lib.isi_code_query_rows_f32(z.data_ptr(), D, codebook.data_ptr(), rows.data_ptr(), Q * cells, K, D, stream),
                   "isi_code_query_rows_f32")

    def torch_rows():
        r = torch.cdist(z.reshape(Q * cells, D), codebook).square_().view(Q, cells, K)
        return r.gather(2, one_item.expand(Q, cells).unsqueeze(-1))

    def hard(handle=lib, out="hard"):
        rc = handle.isi_code_search_f32(codes.data_ptr(), query.data_ptr(), weights.data_ptr(), table.data_ptr(), None,
                                        dist[out].data_ptr(), N, cells, K, Q, 0, workspace.data_ptr(), workspace.numel() * 4, stream)
        assert rc == 0, handle.isi_last_error()

    def soft(source=None):
        source = rows if source is None else source
        _hip.check(lib.isi_code_search_rows_f32(codes.data_ptr(), source.data_ptr(), weights.data_ptr(), None,
                                                dist["soft"].data_ptr(), N, cells, K, Q, 0, workspace.data_ptr(),
                                                workspace.numel() * 4, stream), "isi_code_search_rows_f32")

    # the shifted pair: the window is the first W columns of the same queries
    wq = query[:, :, :W].contiguous()
    ww = weights[:, :, :W].contiguous()
    wrows = rows.view(Q, F, T, K)[:, :, :W].reshape(Q, F * W, K)
    wgathered = table[wq.reshape(Q, F * W).long()].contiguous()
    sdist = {k: torch.empty(Q, count, N, dtype=torch.float32, device=dev) for k in ("hard", "soft", "parent")}
    sneed = lib.isi_code_shift_search_workspace_bytes(N, F, T, W, count, K, Q)
    sworkspace = torch.empty((sneed + 3) // 4, dtype=torch.float32, device=dev)

    def shift_hard(handle=lib, out="hard"):
        rc = handle.isi_code_shift_search_f32(codes.data_ptr(), wq.data_ptr(), ww.data_ptr(), table.data_ptr(),
                                              sdist[out].data_ptr(), N, F, T, W, 0, step, count, K, Q, 0, sworkspace.data_ptr(),
                                              sworkspace.numel() * 4, stream)
        assert rc == 0, handle.isi_last_error()

    def shift_soft(source):
        _hip.check(lib.isi_code_shift_search_rows_f32(codes.data_ptr(), source.data_ptr(), ww.data_ptr(), sdist["soft"].data_ptr(),
                                                      N, F, T, W, 0, step, count, K, Q, 0, sworkspace.data_ptr(),
                                                      sworkspace.numel() * 4, stream), "isi_code_shift_search_rows_f32")

    # ---- the gate: nothing is timed unless the gathered-rows searches give the hard searches' bits at this size
    build()
    hard()
    soft(gathered)
    shift_hard()
    shift_soft(wgathered)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int32)                              # noqa: E731
    if not torch.equal(bits(dist["soft"]), bits(dist["hard"])):
        raise SystemExit(f"{name} Q={Q}: isi_code_search_rows_f32 on gathered table rows differs from isi_code_search_f32: not timed")
    if not torch.equal(bits(sdist["soft"]), bits(sdist["hard"])):
        raise SystemExit(f"{name} Q={Q}: isi_code_shift_search_rows_f32 on gathered table rows differs from "
                         "isi_code_shift_search_f32: not timed")
    if parent is not None:
        hard(parent, "parent")
        shift_hard(parent, "parent")
        torch.cuda.synchronize()
        if not (torch.equal(bits(dist["parent"]), bits(dist["hard"])) and torch.equal(bits(sdist["parent"]), bits(sdist["hard"]))):
            raise SystemExit(f"{name} Q={Q}: the parent library's hard searches give other bits: not timed")
    wrows = wrows.contiguous()
    del gathered, wgathered
    aligned = {"rows": build, "torch_rows": torch_rows, "hard": hard, "soft": soft, "hard_again": hard}
    shifted = {"shift_hard": shift_hard, "shift_soft": lambda: shift_soft(wrows), "shift_hard_again": shift_hard}
    if parent is not None:
        aligned["hard_parent"] = lambda: hard(parent, "parent")
        shifted["shift_hard_parent"] = lambda: shift_hard(parent, "parent")
    res = {"layer": name, "N": N, "F": F, "T": T, "cells": cells, "K": K, "D": D, "Q": Q,
           "rows_MB": round(rows.numel() * 4 / 1e6, 1), "table_MB": round(table.numel() * 4 / 1e6, 2),
           "gathered_rows_bitwise_equal_to_the_hard_searches": True, "parent_library_bitwise_equal": parent is not None or None,
           "aligned": _alternate(aligned, rounds, iters),
           "shifted": {"W": W, "step": step, "S": count, **_alternate(shifted, rounds, iters)}}
    _ratios(res["aligned"], "hard", "soft", "hard_again", "hard_parent")
    _ratios(res["shifted"], "shift_hard", "shift_soft", "shift_hard_again", "shift_hard_parent")
    a, s = res["aligned"], res["shifted"]
    a["torch_rows_over_rows_median"] = round(a["torch_rows"]["median_ms"] / a["rows"]["median_ms"], 2)
    _note(f"{name} Q={Q}: rows {a['rows']['median_ms']:.3f} ms (torch {a['torch_rows']['median_ms']:.3f}), hard "
          f"{a['hard']['median_ms']:.3f}, soft {a['soft']['median_ms']:.3f} (x{a['soft_over_hard_median']}), identical runs differ "
          f"{a['identical_runs_median_difference']:.2%}; shifted hard {s['shift_hard']['median_ms']:.3f}, soft "
          f"{s['shift_soft']['median_ms']:.3f} (x{s['soft_over_hard_median']})"
          + (f"; hard / parent {a['hard_over_parent_median']}, shifted {s['hard_over_parent_median']}" if parent is not None else ""))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libisi_hip.so built from the parent commit (hard searches re-timed against it)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--items", type=int, default=305979)
    ap.add_argument("--codes", type=int, default=512)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "code_search_soft.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    N, K = args.items, args.codes
    g = torch.Generator(device=dev).manual_seed(0)
    codebook = torch.randn(K, D, generator=g, device=dev)
    table = torch.empty(K, K, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().isi_code_distance_table_f32(codebook.data_ptr(), table.data_ptr(), K, D,
                                                      C.c_void_p(_hip.stream_ptr(dev))), "isi_code_distance_table_f32")
    parent = _parent(args.parent_lib)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "unit": "ms per call (device events)",
           "method": f"synthetic uniform codes; all candidates of a case alternate in one run after a warm-up: {args.rounds} rounds "
                     f"of {args.iters} repetitions each; spread = min..max of a candidate's rounds; hard and hard_again are the "
                     "same call (their difference is the run-to-run spread); gathered-rows results compared bitwise with the "
                     "hard searches before anything is timed",
           "parent_library_timed": parent is not None, "cases": []}
    for name, F, T, W, step, queries in (("top", 16, 64, 16, 1, (1, 8)), ("bottom", 32, 128, 32, 2, (1, 8))):
        codes = torch.randint(0, K, (N, F, T), generator=g, device=dev, dtype=torch.int16)
        for Q in queries:
            res["cases"].append(case(dev, parent, name, codes, table, codebook, Q, args.rounds, args.iters, 10 * Q + len(name),
                                     W, step, 49))
        del codes
        torch.cuda.empty_cache()
    moved = [f"{c['layer']} Q={c['Q']} {kind}" for c in res["cases"] for kind in ("aligned", "shifted")
             if c[kind].get("parent_median_inside_identical_runs_min_max") is False]
    res["hard_searches_inside_the_identical_runs_spread"] = (not moved) if parent is not None else None
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    if moved:
        _note("THE HARD SEARCHES MOVED AGAINST THE PARENT LIBRARY: its median lies outside the min..max of two identical runs in "
              + ", ".join(moved))
        sys.exit(3)


if __name__ == "__main__":
    main()
