#!/usr/bin/env python3
"""True-envelope formant correction (csrc/formant.hip; GANsynth_pytorch/stretch.py, bend.py) -- in ONE run:
  kernel          isi_formant_shift_f32 alone at the flagship front-end's stretched size: F = 1024, T = 250, B = 1 and 64, order
                  36 and 145 (220 Hz and 55 Hz at 16 kHz), 16 iterations, ratio 2^(3/12), on frames of a harmonic tone; by
                  device events (a replayed chain of launches, warm, median of windows -- tools/bench_pitch.py's method).
                  Beside the time: the kernel's own count of 2 I n (F + 1) fused multiply-adds per frame, and that count over
                  the data sheet's fp32 vector rate (a floor nobody expects a kernel that reads LDS twice per fma to reach)
  torch           the same definition as a torch expression on the same box (two matmuls and a maximum per iteration, the
                  cosine matrices built once and not timed), and its largest difference from the kernel's envelope
  stft_stretch    isi_stft_stretch_f32 at the same size (T = 125 -> 250), the kernel in front of this one
  public calls    `transpose` (+3) and `bend` (a 6 Hz, +-50 cent vibrato) of a 4 s sound on the flagship helper (n_fft 2048,
                  hop 512), with and without preserve_formants, alternating
  unchanged       `to_audio`, `to_spectrogram`, `stft_stretch`, `resample` and `warp` through the PARENT commit's library
                  (--parent-lib), alternating with this library's, after checking that both give the same bits
There is no pass or fail bar on a time.  Writes profiles/formant.json.

  python tools/bench_formant.py [--parent-lib PATH] [--rounds 7] [--out profiles/formant.json] [--only-kernel]
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
from bench_resample import FP32_VECTOR_FMA_PS, _note, _timed  # noqa: E402
from bench_spec_splice import _alternate, _library, _parent  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402

F, T, ITERATIONS, L = 1024, 250, 16, 64000
RHO = 2.0 ** (3 / 12)


def tone(n, f0=220.0):
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    return sum(torch.sin(2 * math.pi * f0 * h * t) / h for h in range(1, int(7600 / f0))).float() * 0.2


def frames(B, dev):
    """[B, T, 2F]: the flagship helper's STFT of a harmonic tone, the rows at slightly different pitches"""
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper
    helper = MelSpectrogramsHelper(16000, 2 * F, 512, 2 * F).to(dev)
    x = torch.stack([tone(T * 512, 220.0 * (1 + 0.001 * b)) for b in range(min(B, 4))]).to(dev)
    X, _ = helper._stft(x)
    return X[:, :T].repeat(B // X.shape[0] + 1, 1, 1)[:B].contiguous()


def torch_expression(Y, order, iterations, depth):
    """the definition with matmuls: returns a closure over the prebuilt matrices and the envelope it computes"""
    dev = Y.device
    q, k = torch.arange(order, device=dev, dtype=torch.float64)[:, None], torch.arange(F + 1, device=dev, dtype=torch.float64)[None, :]
    Cm = torch.cos(math.pi * q * k / F)
    omega = torch.full((F + 1,), 2.0, device=dev, dtype=torch.float64)
    omega[0] = omega[F] = 1.0
    mw = (0.5 + 0.5 * torch.cos(math.pi * q[:, 0] / order)) * torch.where(q[:, 0] == 0, 1.0, 2.0)
    Cf = (Cm * omega / (2 * F)).float().t().contiguous()               # [F + 1, n]
    Ci = (Cm * mw[:, None]).float().contiguous()                       # [n, F + 1]

    def run():
        P = Y[..., :F] ** 2 + Y[..., F:] ** 2
        Lg = torch.maximum(0.5 * torch.log(P), 0.5 * torch.log(P.amax(-1, keepdim=True)) - depth)
        Lx = torch.cat([Lg[..., :1], Lg], -1)
        A = Lx
        for _ in range(iterations):
            V = (A @ Cf) @ Ci
            A = torch.maximum(Lx, V)
        return V
    return run


def kernel_cases(dev, rounds):
    from GANsynth_pytorch import stretch
    lib, out = _hip.lib(), []
    table = stretch._cos_table(F, dev)
    depth, max_gain = 80.0 * stretch.DB, 40.0 * stretch.DB
    for B in (1, 64):
        Y = frames(B, dev)
        ratio = torch.full((1, T), RHO, dtype=torch.float32, device=dev)
        res, env = torch.empty_like(Y), torch.empty(B, T, F + 1, device=dev)
        for order in (36, 145):
            def launch(with_env=False):
                _hip.check(lib.isi_formant_shift_f32(Y.data_ptr(), ratio.data_ptr(), 1, table.data_ptr(), res.data_ptr(),
                                                     env.data_ptr() if with_env else None, B, T, F, order, ITERATIONS, depth, max_gain,
                                                     C.c_void_p(_hip.stream_ptr(dev))), "isi_formant_shift_f32")
            t = _chain(launch, rounds)
            fma = 2 * ITERATIONS * order * (F + 1) * B * T
            case = {"B": B, "T": T, "F": F, "order": order, "iterations": ITERATIONS, **t, "fma": fma,
                    "fma_per_frame": 2 * ITERATIONS * order * (F + 1), "Gfma_per_s": round(fma / (t["median_us"] * 1e-6) / 1e9, 1),
                    "fma_floor_us": round(fma / FP32_VECTOR_FMA_PS * 1e6, 3)}
            case["time_over_fma_floor"] = round(t["median_us"] / case["fma_floor_us"], 1)
            expr = torch_expression(Y, order, ITERATIONS, depth)
            want = expr()
            launch(True)
            torch.cuda.synchronize()
            case["torch_expression"] = {"median_us": round(_timed(expr, 10) * 1e3, 2),
                                        "largest_envelope_difference_from_the_kernel_nepers": float((want - env).abs().max())}
            case["torch_expression_over_kernel"] = round(case["torch_expression"]["median_us"] / t["median_us"], 2)
            out.append(case)
            _note(json.dumps(case))
    return out


def stretch_cases(dev, rounds):
    from GANsynth_pytorch import stretch
    lib, out = _hip.lib(), []
    for B in (1, 64):
        X = frames(B, dev)[:, :125].contiguous()
        pos = stretch.stretch_positions(125, factor=2.0).to(dev).unsqueeze(0)
        need = lib.isi_stft_stretch_workspace_bytes(B, 125, F)
        ws, res = torch.empty(need // 4, device=dev), torch.empty(B, T, 2 * F, device=dev)

        def launch():
            _hip.check(lib.isi_stft_stretch_f32(X.data_ptr(), pos.data_ptr(), 1, res.data_ptr(), ws.data_ptr(), need, B, 125, T, F, 512,
                                                C.c_void_p(_hip.stream_ptr(dev))), "isi_stft_stretch_f32")
        case = {"B": B, "T": 125, "T_out": T, "F": F, **_chain(launch, rounds)}
        out.append(case)
        _note(json.dumps(case))
    return out


def public_calls(dev, rounds):
    from GANsynth_pytorch import bend, stretch
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper
    helper = MelSpectrogramsHelper(16000, 2 * F, 512, 2 * F).to(dev)
    x = tone(L).to(dev)
    calls = {"transpose_+3": lambda: stretch.transpose(helper, x, 3),
             "transpose_+3_preserve_formants_order_36": lambda: stretch.transpose(helper, x, 3, preserve_formants=True, formant_order=36),
             "transpose_+3_preserve_formants_pitch_estimated": lambda: stretch.transpose(helper, x, 3, preserve_formants=True),
             "bend_vibrato_6Hz_50cents": lambda: bend.vibrato(helper, x, 6.0, 50.0),
             "bend_vibrato_6Hz_50cents_preserve_formants_order_36": lambda: bend.vibrato(helper, x, 6.0, 50.0, preserve_formants=True, formant_order=36),
             "transpose_+3_again": lambda: stretch.transpose(helper, x, 3)}
    est = max(_timed(fn, 2) for fn in calls.values())
    p = _alternate(calls, rounds, int(min(100, max(3, math.ceil(20.0 / max(est, 1e-3))))))
    p["transpose_preserve_over_plain"] = round(p["transpose_+3_preserve_formants_order_36"]["median_us"] / p["transpose_+3"]["median_us"], 3)
    p["bend_preserve_over_plain"] = round(p["bend_vibrato_6Hz_50cents_preserve_formants_order_36"]["median_us"] / p["bend_vibrato_6Hz_50cents"]["median_us"], 3)
    return p


def unchanged(dev, rounds, parent):
    """the kernels this feature stands on, through this library and the parent commit's"""
    from GANsynth_pytorch import bend, resample, stretch
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper
    helper = MelSpectrogramsHelper(16000, 2 * F, 512, 2 * F).to(dev)
    g = torch.Generator().manual_seed(5)
    x48 = (torch.rand(1, 4 * 48000, generator=g) - 0.5).to(dev)
    audio = (0.1 * torch.randn(1, L, generator=g)).to(dev)
    spec = helper.to_spectrogram(audio)
    X = torch.randn(1, 125, 2 * F, generator=g).to(dev)
    pos = stretch.stretch_positions(125, factor=2.0).to(dev)
    wpos = torch.arange(L, dtype=torch.float64, device=dev) * 0.99 + 0.37
    fns = {"to_audio_4s": lambda: helper.to_audio(spec),
           "to_spectrogram_4s": lambda: helper.to_spectrogram(audio),
           "stft_stretch_T125_F1024_x2": lambda: stretch.stft_stretch(X, pos, 512),
           "resample_48k_to_16k_4s": lambda: resample.resample(x48, 48000, 16000),
           "warp_resample_4s": lambda: bend.warp(audio, wpos)}
    calls = {}
    for name, fn in fns.items():
        calls[name], calls[name + "_again"] = fn, fn
        if parent is not None:
            with _library(parent):
                theirs = fn()
            torch.cuda.synchronize()
            assert torch.equal(theirs, fn()), f"{name}: the parent's library gives other bits"

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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "formant.json"))
    ap.add_argument("--only-kernel", action="store_true", help="a few launches of the B = 64 kernel cases and nothing else: for a counter run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    if args.only_kernel:
        from GANsynth_pytorch import stretch
        Y = frames(64, dev)
        ratio = torch.full((T,), RHO, dtype=torch.float32, device=dev)
        for order in (36, 145, 32, 64):
            stretch.formant_shift(Y, ratio, order)
        torch.cuda.synchronize()
        return
    parent = _parent(args.parent_lib)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "unit": "microseconds per launch / call (device events around a window of back-to-back work, warm: the same buffers "
                   "every time)",
           "floors": {"source": "the data sheet's fp32 vector rate, not measured here", "fp32_vector_fma_per_s": FP32_VECTOR_FMA_PS},
           "parent_library": bool(parent)}
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    with torch.no_grad():
        res["kernel"] = kernel_cases(dev, args.rounds)
        path.write_text(json.dumps(res, indent=1) + "\n")
        res["stft_stretch_same_size"] = stretch_cases(dev, args.rounds)
        path.write_text(json.dumps(res, indent=1) + "\n")
        res["public_calls_4s_flagship_helper"] = public_calls(dev, args.rounds)
        _note(json.dumps(res["public_calls_4s_flagship_helper"]))
        path.write_text(json.dumps(res, indent=1) + "\n")
        res["unchanged_kernels"] = unchanged(dev, args.rounds, parent)
        _note(json.dumps(res["unchanged_kernels"]))
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
