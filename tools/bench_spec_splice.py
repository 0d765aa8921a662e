#!/usr/bin/env python3
"""Phase-locked splice (csrc/spec_splice.hip) at the flagship size -- the mel helper of bench.py (n_fft 2048, hop 512:
F = 1024 bins), T = 128 frames, B = 1 and B = 64 sounds, a hole of 32 frames with ramps of 8 -- in ONE run:
  splice / blend      kernel time of isi_spec_splice_f32 (w_batch 1 and B) and isi_spec_splice_blend_f32 by device events (a
                      replayed chain of launches, warm, median of windows -- tools/bench_pitch.py's method), beside
  floor_us            the bytes the kernel must move (splice: 8 original + 4 a + 4 ph + 8 out per element, + 4 of weights per
                      element of w; blend: 12 per sample) over the HBM rate the guide measured on this machine (6.29 TB/s,
                      not measured here)
  torch_expression    the splice as a torch expression (cummax / cummin for the runs, gathers for the anchors)
  to_audio_spliced / to_audio   the two public calls, alternating; the spliced one includes the STFT of the original
  to_audio_parent     `to_audio` through the PARENT commit's library (--parent-lib), alternating with this library's, after
                      checking that both give the same bits: `to_audio` is meant to be unchanged
There is no pass or fail bar on a time.  Writes profiles/spec_splice.json.

  python tools/bench_spec_splice.py [--parent-lib PATH] [--rounds 9] [--out profiles/spec_splice.json]
"""
import argparse
import ctypes as C
import json
import math
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402
from bench_pitch import _chain  # noqa: E402
from bench_resample import HBM_MEASURED_BPS, _median, _note, _timed  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402

N_FFT, HOP, T = 2048, 512, 128
F = N_FFT // 2
HOLE, RAMP = (40, 72), 8
EPS = 1e-6


def weights(w_batch, dev):
    t = torch.arange(T, dtype=torch.float64)
    d = torch.clamp(torch.maximum(HOLE[0] - t, t - (HOLE[1] - 1)), min=0)
    row = torch.clamp(1.0 - d / (RAMP + 1.0), min=0.0).float()
    return row[None, :, None].expand(w_batch, T, F).contiguous().to(dev)


def torch_expression(xo, a, ph, w, mel):
    """isi_spec_splice_f32's rules in torch (float32, on the device)"""
    B, T_, F2 = xo.shape
    F_ = F2 // 2
    re, im = xo[..., :F_], xo[..., F_:]
    wb = w.expand(B, T_, F_)
    mask = wb > 0
    idx = torch.arange(T_, device=xo.device)[None, :, None].expand(B, T_, F_)
    prev = torch.cat([torch.zeros_like(mask[:, :1]), mask[:, :-1]], 1)
    t0 = torch.cummax(torch.where(mask & ~prev, idx, torch.full_like(idx, -1)), 1).values
    t1 = torch.cummin(torch.where(~mask, idx, torch.full_like(idx, T_)).flip(1), 1).values.flip(1)
    left, right = t0 >= 1, t1 <= T_ - 1
    ia, ib = (t0 - 1).clamp(0, T_ - 1), t1.clamp(0, T_ - 1)
    phio = torch.atan2(im, re)
    phia, psia, phib, psib = phio.gather(1, ia), ph.gather(1, ia), phio.gather(1, ib), ph.gather(1, ib)
    d = (phib - phia) - (psib - psia)
    c = (d - 2 * math.pi * torch.ceil((d - math.pi) / (2 * math.pi))) / (t1 - t0 + 1).float()
    phi = torch.where(left & right, phia + (ph - psia) + (idx - t0 + 1).float() * c,
                      torch.where(left, phia + (ph - psia), torch.where(right, phib - (psib - ph), ph)))
    As = torch.exp(0.5 * torch.log(a.clamp(min=0) + EPS)) if mel else a
    Ao = torch.sqrt(re * re + im * im)
    live = (Ao > 0) & (As > 0)
    mag = torch.where(wb == 1, As, torch.where(live, torch.exp((1 - wb) * torch.log(Ao) + wb * torch.log(As)), torch.zeros_like(As)))
    return torch.cat([torch.where(mask, mag * torch.cos(phi), re), torch.where(mask, mag * torch.sin(phi), im)], -1)


def _parent(path):
    """the parent commit's library, loaded beside this one, with the signatures of every entry point it has"""
    if path is None:
        return None
    handle = C.CDLL(str(pathlib.Path(path).resolve()))
    for name, (res, args) in _hip.SIGNATURES.items():
        if hasattr(handle, name):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
    return handle


class _library:
    """`with _library(handle): ...` -- the package's calls go through `handle` inside the block"""

    def __init__(self, handle):
        self.handle = handle

    def __enter__(self):
        self.own = _hip.lib()
        _hip._lib = self.handle

    def __exit__(self, *exc):
        _hip._lib = self.own
        return False


def _alternate(candidates, rounds, iters):
    for fn in candidates.values():
        _timed(fn, 3)
    times = {name: [] for name in candidates}
    for _ in range(rounds):
        for name, fn in candidates.items():
            times[name].append(_timed(fn, iters))
    return {name: {"median_us": round(statistics.median(v) * 1e3, 2), "min_us": round(min(v) * 1e3, 2),
                   "max_us": round(max(v) * 1e3, 2), "calls_per_window": iters, "windows": rounds} for name, v in times.items()}


def case(B, dev, rounds, parent):
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper
    lib = _hip.lib()
    stream = lambda: C.c_void_p(_hip.stream_ptr(dev))      # asked at every launch: a graph capture runs on its own stream  # noqa: E731
    helper = MelSpectrogramsHelper(16000, N_FFT, HOP, N_FFT).to(dev)
    g = torch.Generator().manual_seed(B)
    audio = (0.1 * torch.randn(B, T * HOP, generator=g)).to(dev)
    spec = helper.to_spectrogram(audio)
    res = {"B": B, "T": T, "F": F, "mel": 1}
    # ---- the kernels, on the arrays the public call hands them
    X_orig, _ = helper._stft(audio)
    _, (_, a, ph) = helper._to_audio(spec, keep=True)
    out = torch.empty_like(X_orig)
    for w_batch in sorted({1, B}):
        w = weights(w_batch, dev)

        def launch():
            _hip.check(lib.isi_spec_splice_f32(X_orig.data_ptr(), a.data_ptr(), ph.data_ptr(), w.data_ptr(), w_batch, out.data_ptr(),
                                               B, T, F, 1, stream()), "isi_spec_splice_f32")
        t = _chain(launch, rounds)
        nbytes = B * T * F * 24 + w_batch * T * F * 4
        want = torch_expression(X_orig, a, ph, w, 1)
        launch()
        torch.cuda.synchronize()
        k = {"kernel": t, "bytes": nbytes, "floor_us": round(nbytes / HBM_MEASURED_BPS * 1e6, 3),
             "max_abs_diff_to_torch_expression": float((want - out).abs().max()), "largest_magnitude": float(want.abs().max())}
        del want
        k["time_over_floor"] = round(t["median_us"] / k["floor_us"], 2)
        k["achieved_TB_per_s"] = round(nbytes / (t["median_us"] * 1e-6) / 1e12, 3)
        k["torch_expression"] = _median(lambda: torch_expression(X_orig, a, ph, w, 1), rounds)
        k["torch_expression_over_kernel"] = round(k["torch_expression"]["median_us"] / t["median_us"], 2)
        res[f"splice_w_batch_{'B' if w_batch == B and B > 1 else 1}"] = k
        _note(json.dumps(k))
    extra = N_FFT // HOP - 1
    touched = torch.zeros(B, T + extra, dtype=torch.uint8, device=dev)
    touched[:, :T] = (weights(1, dev) > 0).any(-1)
    ola, blended = helper.to_audio(spec), torch.empty_like(audio)

    def launch_blend():
        _hip.check(lib.isi_spec_splice_blend_f32(audio.data_ptr(), ola.data_ptr(), touched.data_ptr(), blended.data_ptr(), B, T + extra,
                                                 N_FFT, HOP, T * HOP, stream()), "isi_spec_splice_blend_f32")
    t = _chain(launch_blend, rounds)
    nbytes = B * T * HOP * 12 + B * (T + extra)
    res["blend"] = {"kernel": t, "bytes": nbytes, "floor_us": round(nbytes / HBM_MEASURED_BPS * 1e6, 3)}
    res["blend"]["time_over_floor"] = round(t["median_us"] / res["blend"]["floor_us"], 2)
    res["blend"]["achieved_TB_per_s"] = round(nbytes / (t["median_us"] * 1e-6) / 1e12, 3)
    _note(json.dumps(res["blend"]))
    # ---- the public calls
    w = weights(1, dev)
    calls = {"to_audio": lambda: helper.to_audio(spec), "to_audio_spliced": lambda: helper.to_audio_spliced(spec, audio, w),
             "to_audio_again": lambda: helper.to_audio(spec)}
    if parent is not None:
        with _library(parent):
            theirs = helper.to_audio(spec)
        torch.cuda.synchronize()
        assert torch.equal(theirs, helper.to_audio(spec)), "the parent's library gives other bits for to_audio"

        def through_parent():
            with _library(parent):
                helper.to_audio(spec)
        calls["to_audio_parent"] = through_parent
    est = _timed(calls["to_audio_spliced"], 3)
    res["public_calls"] = _alternate(calls, rounds, int(min(200, max(3, math.ceil(20.0 / max(est, 1e-3))))))
    p = res["public_calls"]
    p["spliced_over_to_audio"] = round(p["to_audio_spliced"]["median_us"] / p["to_audio"]["median_us"], 3)
    p["identical_runs_median_difference"] = round(abs(p["to_audio_again"]["median_us"] - p["to_audio"]["median_us"]) / p["to_audio"]["median_us"], 4)
    if parent is not None:
        p["parent_over_this_to_audio"] = round(p["to_audio_parent"]["median_us"] / p["to_audio"]["median_us"], 4)
        lo = min(p["to_audio"]["min_us"], p["to_audio_again"]["min_us"])
        hi = max(p["to_audio"]["max_us"], p["to_audio_again"]["max_us"])
        p["parent_median_inside_identical_runs_min_max"] = bool(lo <= p["to_audio_parent"]["median_us"] <= hi)
        p["to_audio_bits_equal_parent"] = True
    _note(json.dumps(p))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spec_splice.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    parent = _parent(args.parent_lib)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "unit": "microseconds per launch / call (device events around a window of back-to-back work, warm)",
           "floors": {"source": "HBM rate of the MI355X guide, not measured here", "hbm_bytes_per_s": HBM_MEASURED_BPS},
           "hole": {"frames": list(HOLE), "ramp_frames": RAMP, "bins": "all"}, "parent_library": bool(parent)}
    for B in (1, 64):
        res[f"B{B}"] = case(B, dev, args.rounds, parent)
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
