#!/usr/bin/env python3
"""Phase-locked stretch (csrc/stft_stretch.hip) at the flagship size -- the mel helper of bench.py (n_fft 2048, hop 512:
F = 1024 bins), T = 125 frames, B = 1 and B = 64 sounds, factors 0.5, 1.5 and 2 -- in ONE run:
  call                kernel time of isi_stft_stretch_f32 (both launches) by device events (a replayed chain of launches, warm,
                      median of windows -- tools/bench_pitch.py's method)
  preparation         the same call with T_out = 1 from a fractional position: the preparation pass plus a recursion of one
                      frame; beside it floor_us, the bytes the pass must move (8 read, 16 written per source element) over
                      the HBM rate the guide measured on this machine (6.29 TB/s, not measured here)
  recursion           call - preparation, and per_frame_us = recursion / T_out: the latency of one step of the chain
  per_frame_by_F      the same per-frame latency at F = 64 (one wavefront: the barrier costs nothing), 256 and 1024, B = 1,
                      factor 2: what the barrier and the width add to the dependent chain of one step
  time_stretch / transpose   the public calls on the same sound, alternating with `to_audio` + `to_spectrogram` of it -- the
                      cost scale a user feels
  front_end           `to_audio` and `to_spectrogram` through the PARENT commit's library (--parent-lib), alternating with
                      this library's, after checking that both give the same bits: the existing kernels are meant to be
                      unchanged, and their times should not move beyond the spread of two identical runs
There is no pass or fail bar on a time.  Writes profiles/stft_stretch.json.

  python tools/bench_stft_stretch.py [--parent-lib PATH] [--rounds 9] [--out profiles/stft_stretch.json]
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
from bench_resample import HBM_MEASURED_BPS, _note, _timed  # noqa: E402
from bench_spec_splice import _alternate, _library, _parent  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402

N_FFT, HOP, T = 2048, 512, 125
FACTORS = (0.5, 1.5, 2.0)


def kernel_times(X, hop, factor, rounds):
    """isi_stft_stretch_f32 on X [B, T, 2F]: the whole call, the preparation (T_out = 1), their difference per frame"""
    from GANsynth_pytorch.stretch import stretch_positions
    lib, dev = _hip.lib(), X.device
    B, T_, F = X.shape[0], X.shape[1], X.shape[2] // 2
    need = lib.isi_stft_stretch_workspace_bytes(B, T_, F)
    ws = torch.empty(need // 4, device=dev)
    pos = stretch_positions(T_, factor=factor).to(dev)
    T_out = pos.numel()
    out = torch.empty(B, T_out, 2 * F, device=dev)
    one = torch.full((1,), 0.5, device=dev)

    def launch(p, n):
        _hip.check(lib.isi_stft_stretch_f32(X.data_ptr(), p.data_ptr(), 1, out.data_ptr(), ws.data_ptr(), need, B, T_, n, F, hop,
                                            C.c_void_p(_hip.stream_ptr(dev))), "isi_stft_stretch_f32")
    whole = _chain(lambda: launch(pos, T_out), rounds)
    prep = _chain(lambda: launch(one, 1), rounds)
    nbytes = B * T_ * F * 24
    rec = whole["median_us"] - prep["median_us"]
    return {"B": B, "T": T_, "F": F, "factor": factor, "T_out": T_out, "call": whole, "preparation": prep,
            "preparation_bytes": nbytes, "preparation_floor_us": round(nbytes / HBM_MEASURED_BPS * 1e6, 3),
            "preparation_over_floor": round(prep["median_us"] / (nbytes / HBM_MEASURED_BPS * 1e6), 2),
            "recursion_us": round(rec, 3), "per_frame_us": round(rec / T_out, 4)}


def case(B, dev, rounds, parent):
    from GANsynth_pytorch import stretch
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper
    helper = MelSpectrogramsHelper(16000, N_FFT, HOP, N_FFT).to(dev)
    g = torch.Generator().manual_seed(B)
    n = torch.arange(T * HOP, dtype=torch.float64) / 16000.0
    tone = sum(a * torch.sin(2 * math.pi * 440.0 * k * n) for k, a in ((1, 0.5), (2, 0.25), (3, 0.125))).float()
    audio = (tone[None] + 0.01 * torch.randn(B, T * HOP, generator=g)).to(dev)
    X, _ = helper._stft(audio)
    res = {"B": B, "kernel": []}
    for factor in FACTORS:
        k = kernel_times(X, HOP, factor, rounds)
        res["kernel"].append(k)
        _note(json.dumps(k))
    spec = helper.to_spectrogram(audio)
    calls = {"to_audio_plus_to_spectrogram": lambda: helper.to_spectrogram(helper.to_audio(spec)),
             "time_stretch_2": lambda: stretch.time_stretch(helper, audio, 2.0),
             "time_stretch_0.5": lambda: stretch.time_stretch(helper, audio, 0.5),
             "transpose_+3": lambda: stretch.transpose(helper, audio, 3),
             "transpose_-4": lambda: stretch.transpose(helper, audio, -4),
             "to_audio_plus_to_spectrogram_again": lambda: helper.to_spectrogram(helper.to_audio(spec))}
    est = max(_timed(fn, 2) for fn in calls.values())
    p = _alternate(calls, rounds, int(min(100, max(3, math.ceil(20.0 / max(est, 1e-3))))))
    base = p["to_audio_plus_to_spectrogram"]["median_us"]
    for name in ("time_stretch_2", "time_stretch_0.5", "transpose_+3", "transpose_-4"):
        p[name]["over_to_audio_plus_to_spectrogram"] = round(p[name]["median_us"] / base, 3)
    res["public_calls"] = p
    _note(json.dumps(p))
    # ---- the existing front-end kernels against the parent commit's library
    front = {"to_audio": lambda: helper.to_audio(spec), "to_spectrogram": lambda: helper.to_spectrogram(audio),
             "to_audio_again": lambda: helper.to_audio(spec), "to_spectrogram_again": lambda: helper.to_spectrogram(audio)}
    if parent is not None:
        with _library(parent):
            theirs = helper.to_audio(spec), helper.to_spectrogram(audio)
        torch.cuda.synchronize()
        assert torch.equal(theirs[0], helper.to_audio(spec)) and torch.equal(theirs[1], helper.to_spectrogram(audio)), \
            "the parent's library gives other bits for the front-end"

        def through(fn):
            def run():
                with _library(parent):
                    fn()
            return run
        front["to_audio_parent"] = through(front["to_audio"])
        front["to_spectrogram_parent"] = through(front["to_spectrogram"])
    est = max(_timed(fn, 2) for fn in front.values())
    f = _alternate(front, rounds, int(min(200, max(3, math.ceil(20.0 / max(est, 1e-3))))))
    for name in ("to_audio", "to_spectrogram"):
        f[name + "_identical_runs_median_difference"] = round(abs(f[name + "_again"]["median_us"] - f[name]["median_us"]) / f[name]["median_us"], 4)
        if parent is not None:
            f[name + "_parent_over_this"] = round(f[name + "_parent"]["median_us"] / f[name]["median_us"], 4)
            lo = min(f[name]["min_us"], f[name + "_again"]["min_us"])
            hi = max(f[name]["max_us"], f[name + "_again"]["max_us"])
            f[name + "_parent_median_inside_identical_runs_min_max"] = bool(lo <= f[name + "_parent"]["median_us"] <= hi)
            f[name + "_bits_equal_parent"] = True
    res["front_end"] = f
    _note(json.dumps(f))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stft_stretch.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    parent = _parent(args.parent_lib)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "unit": "microseconds per launch / call (device events around a window of back-to-back work, warm)",
           "floors": {"source": "HBM rate of the MI355X guide, not measured here", "hbm_bytes_per_s": HBM_MEASURED_BPS},
           "parent_library": bool(parent)}
    for B in (1, 64):
        res[f"B{B}"] = case(B, dev, args.rounds, parent)
    g = torch.Generator().manual_seed(7)
    res["per_frame_by_F"] = []
    for F in (64, 256, 1024):
        k = kernel_times(torch.randn(1, T, 2 * F, generator=g).to(dev), F // 2, 2.0, args.rounds)
        res["per_frame_by_F"].append({"F": F, "workgroup": min(1024, (F + 63) // 64 * 64), "per_frame_us": k["per_frame_us"],
                                      "recursion_us": k["recursion_us"], "preparation_us": k["preparation"]["median_us"]})
    _note(json.dumps(res["per_frame_by_F"]))
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
