#!/usr/bin/env python3
"""Time-warped search of the code database at NSynth's size: N = 305 979 stored sounds, K = 512
codes, synthetic uniform codes; whole-map queries against the top maps (F = 16, T = 64), the bottom maps (F = 32, T = 128,
drift in bottom columns) and both (drift in top columns), at drift +-4 and +-8, Q = 1.  Per case, in ONE run, after a
warm-up, the candidates alternating A B C ... B C A ... (the order rotates from round to round):
  warp            isi_code_warp_search_f32 on rows gathered from the code distance table
  shift_rows      isi_code_shift_search_rows_f32 at S = hi - lo + 1 offsets of a window of T - S + 1 columns (both layers:
                  the two accumulated launches): the yardstick -- the same kind of look-up, counted below, without the
                  recurrence and with one sum per offset instead of one per (column, drift)
  torch_warp      the torch expression of the warped distance (gather + a loop over the columns with shifted minima) on
                  --torch-items items, scaled to N by the item count: what a user could write without the kernel
  aligned / aligned_again / aligned_parent    isi_code_search_rows_f32 of this library twice (their difference is the
                  run-to-run spread) and of the PARENT commit's library (--parent-lib)
  shift_again / shift_parent                  the same for isi_code_shift_search_rows_f32
Look-ups are counted from the shapes: warp N V W S (band cells times rows per column, V = sum F r), shift N F r W_s S per
layer; ns per thousand look-ups and the ratio warp / shift are reported.  Device events around `iters` repetitions, median
and min..max of `rounds` rounds.  The tool REFUSES to time a case unless the warped search with the band closed at 0 agrees
with the aligned rows search within the two kernels' bounds, the torch expression agrees with the kernel to 1e-5 relative on
its items, and the parent's library gives this library's bits on the existing searches.  Where the parent library's median
lies outside the min..max of the two identical runs, the tool says so loudly, still writes the record and exits with
status 3.  Writes profiles/code_search_warp.json (an existing retrieval_experiment entry, written by
tools/warp_retrieval_experiment.py, is kept).

  python tools/bench_code_warp.py [--parent-lib PATH] [--rounds 8] [--iters 3] [--items 305979] [--torch-items 2048] [--out ...]
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
OLD_SYMBOLS = ("isi_code_search_rows_f32", "isi_code_shift_search_rows_f32", "isi_code_search_workspace_bytes",
               "isi_code_shift_search_workspace_bytes", "isi_last_error")


def _note(msg):
    print(f"[bench_code_warp] {msg}", file=sys.stderr, flush=True)


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
    if path is None:
        return None
    handle = C.CDLL(str(pathlib.Path(path).resolve()))
    for name in OLD_SYMBOLS:
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _hip.SIGNATURES[name]
    return handle


def _alternate(candidates, rounds, iters):
    for fn in candidates.values():                                    # warm-up: every candidate, twice
        _timed(fn, 2)
    times = {name: [] for name in candidates}
    names = list(candidates)
    for k in range(rounds):                                           # the order rotates: a candidate's time depends a little
        for name in names[k % len(names):] + names[:k % len(names)]:  # on what ran before it (caches, clocks)
            times[name].append(_timed(candidates[name], iters))
    return {name: _summary(v) for name, v in times.items()}


def torch_warp(layers, lo, hi, items):
    """The warped distance of query 0 to the first `items` stored items, in torch: layers = [(codes int64 [n, F, T r],
    rows [F, W r, K], r)].  cost [n, W, T], then the recurrence column by column on [n, T]."""
    inf = float("inf")
    cost = None
    for codes, rows, r in layers:
        n, F, Tr = codes.shape
        T, W = Tr // r, rows.shape[1] // r
        for u in range(r):
            sub = codes[:items, :, u::r]                                                # [n, F, T]
            picked = torch.gather(rows[None, :, u::r, :].expand(sub.shape[0], F, W, rows.shape[2]), 3,
                                  sub[:, :, None, :].expand(sub.shape[0], F, W, T))     # [n, F, W, T]
            part = picked.sum(1)
            cost = part if cost is None else cost + part
    n, W, T = cost.shape
    drift = torch.arange(T, device=cost.device)[None, :] - torch.arange(W, device=cost.device)[:, None]
    ok = (drift >= lo) & (drift <= hi)
    d = torch.where(ok[0], cost[:, 0], inf)
    pad = torch.full((n, 2), inf, device=cost.device)
    for i in range(1, W):
        wide = torch.cat([pad, d], 1)                                                   # wide[:, t + 2] = d[:, t]
        best = torch.minimum(torch.minimum(wide[:, 1:T + 1], wide[:, 2:]), wide[:, :T])
        d = torch.where(ok[i], cost[:, i] + best, inf)
    return d.min(1).values


def case(dev, parent, name, layers, lo, hi, N, K, rounds, iters, torch_items):
    """layers: [(codes int16 [N, F, T r] on the device, table [K, K], r)], the first one with r == 1."""
    lib = _hip.lib()
    stream = C.c_void_p(_hip.stream_ptr(dev))
    g = torch.Generator(device=dev).manual_seed(17 + len(name) + hi)
    S = hi - lo + 1
    T = layers[0][0].shape[2]
    W = T
    Ws = T - S + 1                                                    # the yardstick's window: S offsets fit
    parts = (_hip.isi_warp_part * len(layers))()
    keep, shift_jobs, aligned_jobs, torch_layers = [], [], [], []
    for p, (codes, table, r) in enumerate(layers):
        F = codes.shape[1]
        query = torch.randint(0, K, (1, F, W * r), generator=g, device=dev)
        rows = table[query.reshape(1, -1)].contiguous()                                 # [1, F W r, K]
        parts[p].codes, parts[p].rows, parts[p].weights = codes.data_ptr(), rows.data_ptr(), None
        parts[p].F, parts[p].r, parts[p].K = F, r, K
        window = rows.view(1, F, W * r, K)[:, :, :Ws * r].reshape(1, F * Ws * r, K).contiguous()
        keep += [query, rows, window]
        shift_jobs.append((codes, window, F, T * r, Ws * r, r))
        aligned_jobs.append((codes, rows, F * T * r))
        torch_layers.append((codes[:torch_items].long(), rows.view(F, W * r, K), r))
    V = sum(layer[0].shape[1] * layer[2] for layer in layers)
    dist = {k: torch.empty(1, N, dtype=torch.float32, device=dev) for k in ("warp", "closed", "aligned", "parent")}
    sdist = {k: torch.empty(1, S, N, dtype=torch.float32, device=dev) for k in ("own", "parent")}
    need = max([lib.isi_code_search_workspace_bytes(N, cells, K, 1) for _, _, cells in aligned_jobs]
               + [lib.isi_code_shift_search_workspace_bytes(N, F, Tr, Wr, S, K, 1) for _, _, F, Tr, Wr, _ in shift_jobs])
    workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)

    def warp(band=(lo, hi), out="warp"):
        _hip.check(lib.isi_code_warp_search_f32(parts, len(layers), None, dist[out].data_ptr(), None, N, T, W, band[0], band[1],
                                                1, stream), "isi_code_warp_search_f32")

    def aligned(handle=lib, out="aligned"):
        for done, (codes, rows, cells) in enumerate(aligned_jobs):
            rc = handle.isi_code_search_rows_f32(codes.data_ptr(), rows.data_ptr(), None, None, dist[out].data_ptr(), N, cells, K, 1,
                                                 int(done > 0), workspace.data_ptr(), workspace.numel() * 4, stream)
            assert rc == 0, handle.isi_last_error()

    def shift(handle=lib, out="own"):
        for done, (codes, window, F, Tr, Wr, r) in enumerate(shift_jobs):
            rc = handle.isi_code_shift_search_rows_f32(codes.data_ptr(), window.data_ptr(), None, sdist[out].data_ptr(), N, F, Tr, Wr,
                                                       0, r, S, K, 1, int(done > 0), workspace.data_ptr(), workspace.numel() * 4,
                                                       stream)
            assert rc == 0, handle.isi_last_error()

    def by_torch():
        return torch_warp(torch_layers, lo, hi, torch_items)

    # ---- the gates
    warp()
    warp((0, 0), "closed")
    aligned()
    shift()
    torch.cuda.synchronize()
    tolerance = (V * W + V + W + 4) * 2.0 ** -24
    if not bool(((dist["closed"] - dist["aligned"]).abs() <= tolerance * dist["aligned"]).all()):
        raise SystemExit(f"{name} +-{hi}: the warped search with the band closed differs from the aligned rows search: not timed")
    expression = by_torch()
    if not torch.allclose(expression, dist["warp"][0, :torch_items], rtol=1e-5, atol=0):
        raise SystemExit(f"{name} +-{hi}: the torch expression differs from the kernel: not timed")
    if not bool((dist["warp"] <= dist["closed"]).all()):
        raise SystemExit(f"{name} +-{hi}: a band wider than the closed one increased a distance: not timed")
    if parent is not None:
        aligned(parent, "parent")
        shift(parent, "parent")
        torch.cuda.synchronize()
        bits = lambda t: t.view(torch.int32)                          # noqa: E731
        if not (torch.equal(bits(dist["parent"]), bits(dist["aligned"])) and torch.equal(bits(sdist["parent"]), bits(sdist["own"]))):
            raise SystemExit(f"{name} +-{hi}: the parent library's searches give other bits: not timed")
    candidates = {"warp": warp, "shift_rows": shift}
    if parent is not None:
        candidates["shift_parent"] = lambda: shift(parent, "parent")
    candidates.update({"shift_again": shift, "aligned": aligned})
    if parent is not None:
        candidates["aligned_parent"] = lambda: aligned(parent, "parent")
    candidates.update({"aligned_again": aligned, "torch_warp": by_torch})
    res = {"layers": name, "N": N, "K": K, "T": T, "W": W, "drift": [lo, hi], "S": S, "products_per_column_V": V,
           "closed_band_within_bounds_of_the_aligned_search": True, "torch_expression_within_1e-5": True,
           "parent_library_bitwise_equal": parent is not None or None, **_alternate(candidates, rounds, iters)}
    warp_lookups = N * V * W * S
    shift_lookups = sum(N * F * Wr * S for _, _, F, _, Wr, _ in shift_jobs)
    w_ms, s_ms = res["warp"]["median_ms"], res["shift_rows"]["median_ms"]
    res["warp_lookups"], res["shift_lookups"], res["shift_window_columns"] = warp_lookups, shift_lookups, Ws
    res["warp_ns_per_1000_lookups"] = round(w_ms * 1e6 / (warp_lookups / 1000), 3)
    res["shift_ns_per_1000_lookups"] = round(s_ms * 1e6 / (shift_lookups / 1000), 3)
    res["warp_over_shift_per_lookup"] = round(res["warp_ns_per_1000_lookups"] / res["shift_ns_per_1000_lookups"], 3)
    res["torch_warp_scaled_to_N_ms"] = round(res["torch_warp"]["median_ms"] * N / torch_items, 2)
    res["torch_over_warp"] = round(res["torch_warp_scaled_to_N_ms"] / w_ms, 1)
    for own, again, old in (("aligned", "aligned_again", "aligned_parent"), ("shift_rows", "shift_again", "shift_parent")):
        lo_ms, hi_ms = min(res[own]["min_ms"], res[again]["min_ms"]), max(res[own]["max_ms"], res[again]["max_ms"])
        res[own + "_identical_runs_min_max_ms"] = [lo_ms, hi_ms]
        if old in res:
            res[own + "_over_parent_median"] = round(res[own]["median_ms"] / res[old]["median_ms"], 4)
            res[own + "_parent_median_inside_identical_runs_min_max"] = bool(lo_ms <= res[old]["median_ms"] <= hi_ms)
    _note(f"{name} +-{hi}: warp {w_ms:.3f} ms, shift_rows {s_ms:.3f} ms, per look-up x{res['warp_over_shift_per_lookup']}; torch "
          f"{res['torch_warp_scaled_to_N_ms']} ms scaled (x{res['torch_over_warp']}); aligned {res['aligned']['median_ms']:.3f}"
          + (f" (parent {res['aligned_parent']['median_ms']:.3f}), shift parent {res['shift_parent']['median_ms']:.3f}"
             if parent is not None else ""))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libisi_hip.so built from the parent commit (existing searches re-timed)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--items", type=int, default=305979)
    ap.add_argument("--torch-items", type=int, default=2048)
    ap.add_argument("--codes", type=int, default=512)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "code_search_warp.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    N, K = args.items, args.codes
    torch_items = min(args.torch_items, N)
    g = torch.Generator(device=dev).manual_seed(0)
    codebook = torch.randn(K, D, generator=g, device=dev)
    table = torch.empty(K, K, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().isi_code_distance_table_f32(codebook.data_ptr(), table.data_ptr(), K, D,
                                                      C.c_void_p(_hip.stream_ptr(dev))), "isi_code_distance_table_f32")
    parent = _parent(args.parent_lib)
    top = torch.randint(0, K, (N, 16, 64), generator=g, device=dev, dtype=torch.int16)
    bottom = torch.randint(0, K, (N, 32, 128), generator=g, device=dev, dtype=torch.int16)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "unit": "ms per call, Q = 1 (device events)",
           "method": f"synthetic uniform codes; all candidates of a case alternate in one run after a warm-up, in rotating order: {args.rounds} rounds "
                     f"of {args.iters} repetitions each; spread = min..max of a candidate's rounds; X and X_again are the same "
                     f"call; torch_warp runs on {torch_items} items and is scaled by the item count",
           "parent_library_timed": parent is not None, "cases": []}
    for name, layers in (("top", [(top, table, 1)]), ("bottom", [(bottom, table, 1)]), ("both", [(top, table, 1), (bottom, table, 2)])):
        for half in (4, 8):
            res["cases"].append(case(dev, parent, name, layers, -half, half, N, K, args.rounds, args.iters, torch_items))
            torch.cuda.empty_cache()
    moved = [f"{c['layers']} +-{c['drift'][1]} {kind}" for c in res["cases"] for kind in ("aligned", "shift_rows")
             if c.get(kind + "_parent_median_inside_identical_runs_min_max") is False]
    res["existing_searches_inside_the_identical_runs_spread"] = (not moved) if parent is not None else None
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    if path.exists():
        old = json.loads(path.read_text())
        if "retrieval_experiment" in old:
            res["retrieval_experiment"] = old["retrieval_experiment"]
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    if moved:
        _note("THE EXISTING SEARCHES MOVED AGAINST THE PARENT LIBRARY: its median lies outside the min..max of two identical runs in "
              + ", ".join(moved))
        sys.exit(3)


if __name__ == "__main__":
    main()
