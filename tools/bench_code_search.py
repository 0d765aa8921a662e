#!/usr/bin/env python3
"""Query-by-example search of the code database (csrc/code_search.hip) at NSynth's size: N = 305 979 stored sounds, K = 512,
top maps of 1024 cells and bottom maps of 4096, Q = 1 and Q = 8 queries, synthetic uniform codes.  Per case: the time of one
isi_code_search_f32 call (its two launches: the search and the fixed-order reduction of the per-split sums; device events
around `iters` calls), the bytes of codes it streams per second (N C 2 Q bytes per call: every query reads the codes again),
the table look-ups per second (N C Q), and -- on the same box, in the same run, the two candidates alternating A B A B --
the torch expression a user would otherwise write, `table[q[None, :], codes.long()].mul(w).sum(1)` per query (its
`codes.long()` is counted: the database is stored as uint16).  Also the one-off costs: `CodeIndex.from_arrays` from host
arrays (validation + upload) and the two distance tables.  Results are compared before anything is timed.
Writes profiles/code_search.json.

  python tools/bench_code_search.py [--rounds 5] [--iters 20] [--torch-iters 2] [--items 305979] [--out profiles/code_search.json]
"""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
import torch  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402

COPY_TBPS = 5.3           # what a device-to-device copy reaches on this part


def _note(msg):
    print(f"[bench_code_search] {msg}", file=sys.stderr, flush=True)


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


def search_case(dev, codes, table, Q, rounds, iters, torch_iters, seed):
    """codes int16 [N, C] on the device (uint16 bit patterns below 2^15)."""
    lib = _hip.lib()
    N, cells = codes.shape
    K = table.shape[0]
    g = torch.Generator(device=dev).manual_seed(seed)
    query = torch.randint(0, K, (Q, cells), generator=g, device=dev, dtype=torch.int16)
    weights = torch.rand(Q, cells, generator=g, device=dev) * 2.0
    dist = torch.empty(Q, N, dtype=torch.float32, device=dev)
    need = lib.isi_code_search_workspace_bytes(N, cells, K, Q)
    workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    stream = C.c_void_p(_hip.stream_ptr(dev))

    def ours():
        _hip.check(lib.isi_code_search_f32(codes.data_ptr(), query.data_ptr(), weights.data_ptr(), table.data_ptr(), None,
                                           dist.data_ptr(), N, cells, K, Q, 0, workspace.data_ptr(), need, stream),
                   "isi_code_search_f32")

    out_torch = torch.empty(Q, N, dtype=torch.float32, device=dev)

    def expression():
        for j in range(Q):
            out_torch[j] = table[query[j].long()[None, :], codes.long()].mul(weights[j]).sum(1)

    ours()
    expression()
    torch.cuda.synchronize()
    rel = float(((dist - out_torch).abs() / out_torch.abs().clamp(min=1e-30)).max())
    assert rel < 1e-4, f"the two candidates disagree: max relative difference {rel}"
    _timed(ours, max(3, iters // 4))
    times = {"isi_code_search_f32": [], "torch_expression": []}
    for _ in range(rounds):
        times["isi_code_search_f32"].append(_timed(ours, iters))
        times["torch_expression"].append(_timed(expression, torch_iters))
    res = {"N": N, "C": cells, "K": K, "Q": Q, "workspace_MB": round(need / 1e6, 1),
           "max_relative_difference_of_the_two": rel, **{k: _summary(v) for k, v in times.items()}}
    ms = res["isi_code_search_f32"]["median_ms"]
    res["code_bytes_streamed_TBps"] = round(N * cells * 2 * Q / ms / 1e9, 3)
    res["fraction_of_copy_rate"] = round(res["code_bytes_streamed_TBps"] / COPY_TBPS, 3)
    res["lookups_per_second_T"] = round(N * cells * Q / ms / 1e9, 3)
    res["torch_over_ours"] = round(res["torch_expression"]["median_ms"] / ms, 2)
    _note(f"C={cells} Q={Q}: {ms:.3f} ms, {res['code_bytes_streamed_TBps']} TB/s of codes, "
          f"{res['lookups_per_second_T']} T look-ups/s, torch {res['torch_expression']['median_ms']:.3f} ms")
    return res


def one_off(dev, top, bottom, K):
    """`CodeIndex.from_arrays` from host uint16 arrays, then the two tables (first call of each)."""
    from interactive_spectrogram_inpainting.utils.datasets.code_index import CodeIndex
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    vq = VQVAE(in_channel=2, num_embeddings=K).to(dev).eval()
    host_top, host_bottom = top.cpu().view(torch.uint16), bottom.cpu().view(torch.uint16)
    N = host_top.shape[0]
    attrs = {"pitch": torch.arange(N) % 128, "instrument_family_str": torch.arange(N) % 11}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = CodeIndex.from_arrays(host_top.view(N, 32, -1), host_bottom.view(N, 64, -1), attrs, vq, dev)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    index.table("top")                      # loads the code object
    index._tables.clear()
    out = {"from_arrays_s": round(build_s, 3), "from_arrays_bytes": int(host_top.numel() + host_bottom.numel()) * 2}
    for layer in ("top", "bottom"):
        out[f"table_{layer}_ms"] = round(_timed(lambda: (index._tables.pop(layer, None), index.table(layer)), 20), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--items", type=int, default=305979)
    ap.add_argument("--codes", type=int, default=512)
    ap.add_argument("--skip-one-off", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "code_search.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    N, K = args.items, args.codes
    g = torch.Generator(device=dev).manual_seed(0)
    top = torch.randint(0, K, (N, 1024), generator=g, device=dev, dtype=torch.int16)
    bottom = torch.randint(0, K, (N, 4096), generator=g, device=dev, dtype=torch.int16)
    codebook = torch.randn(K, 64, generator=g, device=dev)
    table = torch.empty(K, K, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().isi_code_distance_table_f32(codebook.data_ptr(), table.data_ptr(), K, 64,
                                                      C.c_void_p(_hip.stream_ptr(dev))), "isi_code_distance_table_f32")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "unit": "ms per call (device events)",
           "method": f"synthetic uniform codes; the two candidates alternate A B A B ...: {args.rounds} rounds of {args.iters} "
                     f"calls of isi_code_search_f32 (search + reduce launches) and {args.torch_iters} evaluations of the torch "
                     "expression; spread = min..max of a candidate's rounds; results compared before timing",
           "copy_rate_TBps_for_reference": COPY_TBPS, "cases": []}
    for name, codes in (("top", top), ("bottom", bottom)):
        for Q in (1, 8):
            res["cases"].append({"layer": name, **search_case(dev, codes, table, Q, args.rounds, args.iters,
                                                              args.torch_iters, 10 * Q + len(name))})
    if not args.skip_one_off:
        res["one_off"] = one_off(dev, top, bottom, K)
        _note(f"one-off: {res['one_off']}")
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
