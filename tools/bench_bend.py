#!/usr/bin/env python3
"""Time-warped read (csrc/warp_resample.hip) and pitch bending (GANsynth_pytorch/bend.py) -- in ONE run:
  kernel          isi_warp_resample_f32 on rows of L = 64 000 samples (4 s at the models' rate), B = 1 and B = 64, read at
                  rate 1 (64 000 outputs, cut ROLLOFF: 135 taps each) and at rate 2 (32 000 outputs, cut ROLLOFF / 2: 271 taps),
                  from a fractional start, by device events (a replayed chain of launches, warm, median of windows --
                  tools/bench_pitch.py's method).  Beside the time: the taps evaluated, the bytes in and out, and two floors
                  from the MI355X guide's figures (not measured here): the bytes over the HBM rate, and the taps times the
                  OPS_PER_TAP fp32 vector operations the kernel spends on a tap (the weights are evaluated, not looked up)
                  over the fp32 vector rate
  torch           the same sum as a torch expression, B = 1: gather of every output's support times weights evaluated with
                  torch.sinc / torch.special.i0 in float32 -- the alternative a reader would write; and its largest
                  difference from the kernel
  bend            `bend` (a 6 Hz, +-50 cent vibrato) end to end on the flagship helper (n_fft 2048, hop 512), alternating with
                  `transpose` (+1 semitone) and `time_stretch` (x 1.06) of the same 4 s sound
  unchanged       `resample` 48 -> 16 kHz, `stft_stretch` and the two pitch kernels through the PARENT commit's library
                  (--parent-lib), alternating with this library's, after checking that both give the same bits
There is no pass or fail bar on a time.  Writes profiles/bend.json.

  python tools/bench_bend.py [--parent-lib PATH] [--rounds 7] [--out profiles/bend.json]
"""
import argparse
import ctypes as C
import json
import math
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402
from bench_pitch import _chain  # noqa: E402
from bench_resample import FP32_VECTOR_FMA_PS, HBM_MEASURED_BPS, _note, _timed  # noqa: E402
from bench_spec_splice import _alternate, _library, _parent  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402

L = 64000
OPS_PER_TAP = 74      # vector instructions in the tap loop of the compiled kernel: 33 fma, the IEEE division's 12, 29 others


def torch_expression(x, pos, cut):
    """x [1, L] float32, pos [N] float64, cut [N] float32 -> [1, N]: gather of the support times weights"""
    from GANsynth_pytorch.resample import BETA, Z
    reach = int(math.ceil(Z / float(cut.min()))) + 1
    ip = pos.floor()
    k = torch.arange(-reach, reach + 1, device=x.device)
    m = ip.long()[:, None] - k[None, :]
    t = (cut.double()[:, None] * (pos[:, None] - m)).float()
    inside = (t.abs() < Z) & (m >= 0) & (m < x.shape[1])
    u = (1.0 - (t / Z) ** 2).clamp(min=0.0)
    w = cut[:, None] * torch.sinc(t) * torch.special.i0(BETA * u.sqrt()) / torch.special.i0(torch.tensor(BETA, device=x.device))
    return (torch.where(inside, w, torch.zeros_like(w)) * x[0][m.clamp(0, x.shape[1] - 1)]).sum(1)[None]


def kernel_cases(dev, rounds):
    from GANsynth_pytorch.bend import warp
    from GANsynth_pytorch.resample import ROLLOFF
    lib, out = _hip.lib(), []
    for rate in (1, 2):
        N = L // rate
        pos = torch.arange(N, dtype=torch.float64, device=dev) * rate + 0.37
        cut = torch.full((N,), ROLLOFF / rate, dtype=torch.float32, device=dev)
        taps = 2 * int(64.0 / float(cut[0])) + 1
        for B in (1, 64):
            x = torch.rand(B, L, device=dev) - 0.5
            y = torch.empty(B, N, device=dev)

            def launch():
                _hip.check(lib.isi_warp_resample_f32(x.data_ptr(), L, pos.data_ptr(), cut.data_ptr(), 1, y.data_ptr(), N, B, L, N,
                                                     C.c_void_p(_hip.stream_ptr(dev))), "isi_warp_resample_f32")
            t = _chain(launch, rounds)
            nbytes = 4 * B * (L + N) + 12 * N
            n_taps = B * N * taps
            case = {"L": L, "B": B, "rate": rate, "N_out": N, "cut": round(float(cut[0]), 6), "taps_per_output": taps, **t,
                    "taps": n_taps, "bytes_in_plus_out": nbytes, "hbm_floor_us": round(nbytes / HBM_MEASURED_BPS * 1e6, 3),
                    "vector_ops_per_tap": OPS_PER_TAP, "vector_floor_us": round(n_taps * OPS_PER_TAP / FP32_VECTOR_FMA_PS * 1e6, 3),
                    "Gtaps_per_s": round(n_taps / (t["median_us"] * 1e-6) / 1e9, 2)}
            case["time_over_larger_floor"] = round(t["median_us"] / max(case["hbm_floor_us"], case["vector_floor_us"]), 2)
            case["public_call_median_us"] = round(_timed(lambda: warp(x, pos, cut), 20) * 1e3, 2)
            if B == 1:
                want = torch_expression(x, pos, cut)
                launch()
                torch.cuda.synchronize()
                case["torch_expression"] = {"median_us": round(_timed(lambda: torch_expression(x, pos, cut), 10) * 1e3, 2),
                                            "largest_difference_from_the_kernel": float((want - y).abs().max())}
                case["torch_expression_over_kernel"] = round(case["torch_expression"]["median_us"] / t["median_us"], 1)
            out.append(case)
            _note(json.dumps(case))
    return out


def public_calls(dev, rounds):
    from GANsynth_pytorch import bend, stretch
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper
    helper = MelSpectrogramsHelper(16000, 2048, 512, 2048).to(dev)
    n = torch.arange(L, dtype=torch.float64) / 16000.0
    tone = sum(a * torch.sin(2 * math.pi * 440.0 * k * n) for k, a in ((1, 0.5), (2, 0.25), (3, 0.125))).float().to(dev)
    calls = {"transpose_+1": lambda: stretch.transpose(helper, tone, 1),
             "time_stretch_1.06": lambda: stretch.time_stretch(helper, tone, 1.06),
             "bend_vibrato_6Hz_50cents": lambda: bend.vibrato(helper, tone, 6.0, 50.0),
             "bend_glide_0_to_3": lambda: bend.glide(helper, tone, 0.0, 3.0),
             "transpose_+1_again": lambda: stretch.transpose(helper, tone, 1)}
    est = max(_timed(fn, 2) for fn in calls.values())
    p = _alternate(calls, rounds, int(min(100, max(3, math.ceil(20.0 / max(est, 1e-3))))))
    for name in ("bend_vibrato_6Hz_50cents", "bend_glide_0_to_3"):
        p[name]["over_transpose"] = round(p[name]["median_us"] / p["transpose_+1"]["median_us"], 3)
    return p


def unchanged(dev, rounds, parent):
    """the kernels this feature stands on, through this library and the parent commit's"""
    from GANsynth_pytorch import pitch, resample, stretch
    g = torch.Generator().manual_seed(5)
    x48 = (torch.rand(1, 4 * 48000, generator=g) - 0.5).to(dev)
    X = torch.randn(1, 125, 2048, generator=g).to(dev)
    pos = stretch.stretch_positions(125, factor=1.5).to(dev)

    def yin():
        d, e = pitch.difference(x48)
        return pitch.pick(d) + (d, e)
    fns = {"resample_48k_to_16k_4s": lambda: resample.resample(x48, 48000, 16000),
           "stft_stretch_T125_F1024_x1.5": lambda: stretch.stft_stretch(X, pos, 512),
           "pitch_difference_plus_pick_4s": yin}
    calls = {}
    for name, fn in fns.items():
        calls[name], calls[name + "_again"] = fn, fn
        if parent is not None:
            with _library(parent):
                theirs = fn()
            torch.cuda.synchronize()
            ours = fn()
            same = all(torch.equal(a, b) for a, b in zip(theirs, ours)) if isinstance(ours, tuple) else torch.equal(theirs, ours)
            assert same, f"{name}: the parent's library gives other bits"

            def through(f=fn):
                with _library(parent):
                    f()
            calls[name + "_parent"] = through
    est = max(_timed(fn, 2) for fn in calls.values())
    f = _alternate(calls, rounds, int(min(200, max(3, math.ceil(20.0 / max(est, 1e-3))))))
    for name in fns:
        f[name + "_identical_runs_median_difference"] = round(abs(f[name + "_again"]["median_us"] - f[name]["median_us"]) / f[name]["median_us"], 4)
        if parent is not None:
            f[name + "_parent_over_this"] = round(f[name + "_parent"]["median_us"] / f[name]["median_us"], 4)
            f[name + "_bits_equal_parent"] = True
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bend.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    parent = _parent(args.parent_lib)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "unit": "microseconds per launch / call (device events around a window of back-to-back work, warm: the same buffers "
                   "every time, so a 256 KB row is served from cache)",
           "floors": {"source": "figures of the MI355X guide, not measured here", "hbm_bytes_per_s": HBM_MEASURED_BPS,
                      "fp32_vector_ops_per_s_data_sheet": FP32_VECTOR_FMA_PS},
           "parent_library": bool(parent)}
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    res["kernel"] = kernel_cases(dev, args.rounds)
    path.write_text(json.dumps(res, indent=1) + "\n")
    with torch.no_grad():
        res["public_calls_4s_flagship_helper"] = public_calls(dev, args.rounds)
        _note(json.dumps(res["public_calls_4s_flagship_helper"]))
        path.write_text(json.dumps(res, indent=1) + "\n")
        res["unchanged_kernels"] = unchanged(dev, args.rounds, parent)
        _note(json.dumps(res["unchanged_kernels"]))
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
