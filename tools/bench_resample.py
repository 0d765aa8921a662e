#!/usr/bin/env python3
"""Sample-rate conversion (csrc/resample.hip, GANsynth_pytorch/resample.py): kernel time of isi_resample_f32 by device
events (a replayed chain of launches), warm, and the time of the public `resample` call, for 4 s and 60 s clips,
48000 -> 16000 and 44100 -> 16000, B = 1 and B = 64, each beside two floors computed from the MI355X guide's figures
(not measured here):
  hbm_floor_us   bytes in + out over the HBM rate (6.29 TB/s measured float4 copy; 8.0 TB/s on the data sheet)
  fma_floor_us   N_out * taps fused multiply-adds over the fp32 vector rate (157.3 TFLOP/s = 78.65 T fma/s, data sheet)
and, on the same machine, the time of the `to_spectrogram` + `VQVAE.encode` that follows the conversion in /analyze-audio
(B = 1, 65536 samples = 4.1 s: the nearest length whose 128 spectrogram frames the default VQ-VAE's strides divide), so
that a reader sees what share of the route the new stage is.  Writes profiles/resample.json.

  python tools/bench_resample.py [--rounds 9] [--out profiles/resample.json]
"""
import argparse
import json
import math
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
import torch  # noqa: E402
from GANsynth_pytorch import resample as R  # noqa: E402

HBM_MEASURED_BPS = 6.29e12
HBM_SPEC_BPS = 8.0e12
FP32_VECTOR_FMA_PS = 157.3e12 / 2


def _note(msg):
    print(f"[bench_resample] {msg}", file=sys.stderr, flush=True)


def _timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def _median(fn, rounds, window_ms=20.0):
    """Warm up, size a window of about `window_ms` of back-to-back launches, then the median over `rounds` windows."""
    _timed(fn, 3)
    est = _timed(fn, 3)
    iters = int(min(500, max(3, math.ceil(window_ms / max(est, 1e-3)))))
    v = [_timed(fn, iters) for _ in range(rounds)]
    return {"median_us": round(statistics.median(v) * 1e3, 2), "min_us": round(min(v) * 1e3, 2),
            "max_us": round(max(v) * 1e3, 2), "launches_per_window": iters, "windows": rounds}


def _kernel_time(x, fs_in, fs_out, rounds, chain=20):
    """The kernel alone: `chain` launches into one preallocated output, recorded once as a HIP graph (a linear chain)
    and replayed, so that no host launch path sits between them; per launch."""
    import ctypes as C
    from interactive_spectrogram_inpainting import _hip
    orig, new, width, _ = R.geometry(fs_in, fs_out)
    table = R._device_table(fs_in, fs_out, orig, new, x.device)
    B, L = x.shape
    lib = _hip.lib()
    y = torch.empty(B, lib.isi_resample_out_len(L, orig, new), device=x.device)

    def launch():
        _hip.check(lib.isi_resample_f32(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), B, L, orig, new, width,
                                        table.data_ptr(), C.c_void_p(_hip.stream_ptr(x.device))), "isi_resample_f32")
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            launch()
    t = _median(graph.replay, rounds)
    for k in ("median_us", "min_us", "max_us"):
        t[k] = round(t[k] / chain, 3)
    t["launches_per_replay"] = chain
    return t


def resample_cases(dev, rounds):
    out = []
    for fs_in in (48000, 44100):
        orig, new, width, taps = R.geometry(fs_in, 16000)
        for seconds in (4, 60):
            for B in (1, 64):
                L = seconds * fs_in
                x = torch.rand(B, L, device=dev) - 0.5
                n_out = R.resample(x, fs_in, 16000).shape[1]
                t = _kernel_time(x, fs_in, 16000, rounds)
                call = _median(lambda: R.resample(x, fs_in, 16000), rounds)
                t["public_call_median_us"] = call["median_us"]    # allocation + host launch path included when they are longer
                bytes_moved = 4 * B * (L + n_out)
                fmas = B * n_out * taps
                case = {"fs_in": fs_in, "fs_out": 16000, "orig": orig, "new": new, "width": width, "taps": taps,
                        "seconds": seconds, "B": B, "L": L, "N_out": n_out, **t,
                        "bytes_in_plus_out": bytes_moved, "fmas": fmas,
                        "hbm_floor_us": round(bytes_moved / HBM_MEASURED_BPS * 1e6, 3),
                        "hbm_floor_us_at_data_sheet_rate": round(bytes_moved / HBM_SPEC_BPS * 1e6, 3),
                        "fma_floor_us": round(fmas / FP32_VECTOR_FMA_PS * 1e6, 3)}
                case["achieved_Tfma_per_s"] = round(fmas / (t["median_us"] * 1e-6) / 1e12, 3)
                case["time_over_larger_floor"] = round(t["median_us"] / max(case["hbm_floor_us"], case["fma_floor_us"]), 1)
                out.append(case)
                _note(json.dumps(case))
                del x
    return out


def route_after(dev, rounds):
    """What /analyze-audio runs on the converted samples: to_spectrogram + VQVAE.encode, B = 1."""
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    helper = MelSpectrogramsHelper(16000, 2048, 512, 2048).to(dev)
    torch.manual_seed(0)
    vq = VQVAE(in_channel=2).to(dev).eval()
    x = (torch.rand(1, 65536, device=dev) - 0.5) * 0.2
    with torch.no_grad():
        spec = helper.to_spectrogram(x)
        out = {"samples": 65536, "spectrogram": list(spec.shape),
               "to_spectrogram": _median(lambda: helper.to_spectrogram(x), rounds),
               "vqvae_encode": _median(lambda: vq.encode(spec), rounds),
               "to_spectrogram_plus_encode": _median(lambda: vq.encode(helper.to_spectrogram(x)), rounds)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resample.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "unit": "microseconds per launch / call (device events around a window of back-to-back work, warm: the same "
                   "buffers every time, so the 4 s clips are served from cache); median_us of a resample case = the kernel",
           "floors": {"source": "figures of the MI355X guide, not measured here", "hbm_bytes_per_s_measured_copy": HBM_MEASURED_BPS,
                      "hbm_bytes_per_s_data_sheet": HBM_SPEC_BPS, "fp32_vector_fma_per_s_data_sheet": FP32_VECTOR_FMA_PS}}
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    res["resample"] = resample_cases(dev, args.rounds)
    path.write_text(json.dumps(res, indent=1) + "\n")
    res["route_after_resample_B1"] = route_after(dev, args.rounds)
    four = next(c for c in res["resample"] if c["fs_in"] == 48000 and c["seconds"] == 4 and c["B"] == 1)
    res["resample_4s_B1_48k_over_spectrogram_plus_encode"] = round(
        four["median_us"] / res["route_after_resample_B1"]["to_spectrogram_plus_encode"]["median_us"], 4)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
