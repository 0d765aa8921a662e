#!/usr/bin/env python3
"""Pitch estimation (csrc/pitch.hip, GANsynth_pytorch/pitch.py): kernel time of isi_pitch_difference_f32 and of
isi_pitch_pick_f32 by device events (a replayed chain of launches, warm, median of windows -- tools/bench_resample.py's
method), and the time of the public `estimate_pitch` call from 16 kHz audio, for one clip and for 64 clips of 4 s.
Beside each difference-kernel time:
  fma_floor_us    B T (TAU_MAX + 1) W fused multiply-adds over the fp32 vector rate of the MI355X guide (157.3 TFLOP/s =
                  78.65 T fma/s, data sheet; not measured here)
  valu_floor_us   twice that: the specified arithmetic is one subtraction AND one fma per term, two vector instructions
  torch_expression_us (B = 1)  the same function as a torch expression on the same machine: `unfold` the frames and the
                  lagged windows, subtract, square, sum (it materialises B T (TAU_MAX + 1) W floats: 5.8 GB for one clip)
and, on the same machine, `to_spectrogram` + `VQVAE.encode` of a 4.1 s clip (bench_resample.route_after): what
/analyze-audio runs next.  Writes profiles/pitch.json.

  python tools/bench_pitch.py [--rounds 9] [--out profiles/pitch.json]
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
from bench_resample import FP32_VECTOR_FMA_PS, _median, _note, route_after  # noqa: E402
from GANsynth_pytorch import pitch as P  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402

SECONDS = 4


def _chain(launch, rounds, chain=20):
    """`chain` launches recorded once as a HIP graph (a linear chain) and replayed: per launch."""
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


def torch_expression(x):
    """d [B, T, TAU_MAX + 1] of x [B, L] as a torch expression."""
    frames = x.unfold(1, P.W + P.TAU_MAX, P.HOP)                       # [B, T, W + TAU_MAX]
    lagged = frames.unfold(2, P.W, 1)                                  # [B, T, TAU_MAX + 1, W]
    return (frames[:, :, None, :P.W] - lagged).square().sum(-1)


def cases(dev, rounds):
    lib = _hip.lib()
    out = []
    for B in (1, 64):
        L = SECONDS * P.FS_A
        x = torch.rand(B, L, device=dev) - 0.5
        T = lib.isi_pitch_frames(L, P.W, P.HOP, P.TAU_MAX)
        d = torch.empty(B, T, P.TAU_MAX + 1, device=dev)
        e = torch.empty(B, T, device=dev)
        period, ap = torch.empty(B, T, device=dev), torch.empty(B, T, device=dev)

        def difference():
            _hip.check(lib.isi_pitch_difference_f32(x.data_ptr(), L, d.data_ptr(), e.data_ptr(), B, L, P.W, P.HOP, P.TAU_MAX,
                                                    C.c_void_p(_hip.stream_ptr(dev))), "isi_pitch_difference_f32")

        def pick():
            _hip.check(lib.isi_pitch_pick_f32(d.data_ptr(), B * T, P.TAU_MIN, P.TAU_MAX, P.THR, period.data_ptr(),
                                              ap.data_ptr(), C.c_void_p(_hip.stream_ptr(dev))), "isi_pitch_pick_f32")
        t = _chain(difference, rounds)
        fmas = B * T * (P.TAU_MAX + 1) * P.W
        case = {"seconds": SECONDS, "B": B, "L_at_48k": L, "T": T, "difference_kernel": t, "fmas": fmas,
                "fma_floor_us": round(fmas / FP32_VECTOR_FMA_PS * 1e6, 3),
                "valu_floor_us": round(2 * fmas / FP32_VECTOR_FMA_PS * 1e6, 3),
                "pick_kernel": _chain(pick, rounds)}
        case["achieved_Tfma_per_s"] = round(fmas / (t["median_us"] * 1e-6) / 1e12, 3)
        case["time_over_fma_floor"] = round(t["median_us"] / case["fma_floor_us"], 2)
        case["time_over_valu_floor"] = round(t["median_us"] / case["valu_floor_us"], 2)
        audio = torch.rand(B, SECONDS * 16000, device=dev) - 0.5
        case["estimate_pitch_from_16k_public_call"] = _median(lambda: P.estimate_pitch(audio, 16000), rounds)
        if B == 1:
            want = torch_expression(x)
            difference()
            torch.cuda.synchronize()
            case["torch_expression_max_rel_diff"] = float(((want - d).abs() / want.clamp(min=1e-30)).max())
            del want
            case["torch_expression"] = _median(lambda: torch_expression(x), rounds)
            case["torch_expression_over_kernel"] = round(case["torch_expression"]["median_us"] / t["median_us"], 1)
        out.append(case)
        _note(json.dumps(case))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pitch.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "unit": "microseconds per launch / call (device events around a window of back-to-back work, warm)",
           "constants": {"FS_A": P.FS_A, "W": P.W, "HOP": P.HOP, "TAU_MAX": P.TAU_MAX, "TAU_MIN": P.TAU_MIN, "THR": P.THR},
           "floors": {"source": "figures of the MI355X guide, not measured here",
                      "fp32_vector_fma_per_s_data_sheet": FP32_VECTOR_FMA_PS}}
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    res["pitch"] = cases(dev, args.rounds)
    path.write_text(json.dumps(res, indent=1) + "\n")
    res["route_after_B1"] = route_after(dev, args.rounds)
    one = res["pitch"][0]
    res["estimate_pitch_4s_B1_over_spectrogram_plus_encode"] = round(
        one["estimate_pitch_from_16k_public_call"]["median_us"] /
        res["route_after_B1"]["to_spectrogram_plus_encode"]["median_us"], 3)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
