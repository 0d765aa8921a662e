#!/usr/bin/env python3
"""Top-M / palette-restricted codebook search (csrc/vq_topm.hip): kernel time of isi_vq_nearest_topm_f32 by device events
(windows of back-to-back launches, warm, median of windows -- tools/bench_resample.py's method; a launch lasts hundreds
of microseconds, the host's launch path hides behind it) at K = 512, D = 64 for the top and bottom maps of the bench batch
(N = 65 536 and 262 144), M in {1, 4, 8}, without a palette and with one 48-code palette.  Beside each, in the same process:
  exact_kernel        isi_vq_nearest_f32, the exact-fp32 search (one index per vector, plus the quantised vectors, the
                      histogram and the squared error it also writes) at the same N
  torch_expression    torch.cdist(z, E).topk(M, largest=False), the palette as a masked_fill of the [N, K] matrix
Nothing is required of the ratios: they are the measurement DESIGN.md section 6f quotes.  The expectation they confirm or
refute: M = 1 without a palette costs what the exact kernel costs; a larger M adds the maintenance of the sorted list
(5 M vector instructions per distance beside the 32 matrix instructions of a 32-code tile), a palette one bit test per
distance.  Writes profiles/vq_topm.json.

  python tools/bench_vq_topm.py [--rounds 9] [--out profiles/vq_topm.json]
"""
import argparse
import ctypes as C
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402
from bench_resample import _median, _note  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402
from interactive_spectrogram_inpainting.vqvae import _ops  # noqa: E402

D, K = 64, 512
SIZES = {"top_map_B64": 65536, "bottom_map_B64": 262144}
RANKS = (1, 4, 8)
PALETTE_CODES = 48
# fp32 matrix pipe: 256 CUs x 4 SIMDs x 64 flop per cycle (v_mfma_f32_32x32x2f32: 4096 flop in 16 passes of 4 cycles) at
# 2.4 GHz = 157 TFLOP/s
MATRIX_F32_FLOPS = 256 * 4 * 64 * 2.4e9


def torch_expression(z, E, M, mask=None):
    d = torch.cdist(z, E)
    if mask is not None:
        d = d.masked_fill(~mask, float("inf"))
    return d.topk(M, dim=1, largest=False)


def cases(dev, rounds):
    lib = _hip.lib()
    stream = C.c_void_p(_hip.stream_ptr(dev))
    g = torch.Generator().manual_seed(0)
    embed = (torch.randn(D, K, generator=g) * 0.7).to(dev)
    codes, e2 = _ops.pack_codebook(embed)
    palette = torch.zeros(1, K, dtype=torch.bool)
    palette[0, torch.randperm(K, generator=g)[:PALETTE_CODES]] = True
    words = _ops.pack_palettes(palette, K, dev)
    out = {}
    for name, N in SIZES.items():
        z = (torch.randn(N, D, generator=g) * 0.8).to(dev)
        idx = torch.empty(N, dtype=torch.int64, device=dev)
        q = torch.empty(N, D, device=dev)
        counts = torch.zeros(K, dtype=torch.int32, device=dev)
        part = torch.empty(lib.isi_vq_num_partials(N), device=dev)

        def exact():
            _hip.check(lib.isi_vq_nearest_f32(z.data_ptr(), codes.data_ptr(), e2.data_ptr(), idx.data_ptr(), q.data_ptr(),
                                              counts.data_ptr(), part.data_ptr(), N, D, K, stream), "isi_vq_nearest_f32")
        flops = 2.0 * N * K * D
        res = {"N": N, "D": D, "K": K, "exact_kernel": _median(exact, rounds),
               "matrix_pipe_floor_us": round(flops / MATRIX_F32_FLOPS * 1e6, 2), "topm": []}
        res["exact_kernel_over_matrix_floor"] = round(res["exact_kernel"]["median_us"] / res["matrix_pipe_floor_us"], 2)
        _note(f"{name}: exact kernel {res['exact_kernel']['median_us']} us (matrix-pipe floor {res['matrix_pipe_floor_us']} us)")
        for M in RANKS:
            ids = torch.empty(M, N, dtype=torch.int64, device=dev)
            dist = torch.empty(M, N, device=dev)
            for with_palette in (False, True):
                def topm():
                    _hip.check(lib.isi_vq_nearest_topm_f32(z.data_ptr(), codes.data_ptr(), e2.data_ptr(),
                                                           words.data_ptr() if with_palette else None, 1 if with_palette else 0,
                                                           None, ids.data_ptr(), N, dist.data_ptr(), N, N, D, K, M, stream),
                               "isi_vq_nearest_topm_f32")
                t = _median(topm, rounds)
                mask = palette.to(dev) if with_palette else None
                want = torch_expression(z, codes, M, mask)
                torch.cuda.synchronize()
                case = {"M": M, "palette_codes": PALETTE_CODES if with_palette else None, "kernel": t,
                        "over_exact_kernel": round(t["median_us"] / res["exact_kernel"]["median_us"], 3),
                        "ids_equal_to_torch_expression": round(float((want.indices.T == ids).float().mean()), 6)}
                if M == 1 and not with_palette:
                    exact()
                    torch.cuda.synchronize()
                    case["rank_0_equals_exact_kernel"] = bool(torch.equal(ids[0], idx))
                del want
                case["torch_expression"] = _median(lambda: torch_expression(z, codes, M, mask), max(3, rounds // 3))
                case["torch_expression_over_kernel"] = round(case["torch_expression"]["median_us"] / t["median_us"], 2)
                res["topm"].append(case)
                _note(f"{name}: {json.dumps(case)}")
        base = {(c["M"], c["palette_codes"]): c["kernel"]["median_us"] for c in res["topm"]}
        res["account_us"] = {
            "distances_M1_no_palette": base[(1, None)],
            "list_maintenance_M4": round(base[(4, None)] - base[(1, None)], 2),
            "list_maintenance_M8": round(base[(8, None)] - base[(1, None)], 2),
            "palette_M1": round(base[(1, PALETTE_CODES)] - base[(1, None)], 2),
            "palette_M8": round(base[(8, PALETTE_CODES)] - base[(8, None)], 2)}
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vq_topm.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "unit": "microseconds per launch / call (device events around a window of back-to-back work, warm)",
           "floors": {"matrix_f32_flops_per_s": MATRIX_F32_FLOPS,
                      "source": "peak of the fp32 matrix pipe (256 CUs at 2.4 GHz), not measured here"}}
    res["search_K512_D64"] = cases(dev, args.rounds)
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
