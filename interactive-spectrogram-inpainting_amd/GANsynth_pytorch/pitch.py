"""The pitch of a sound on MI355X: what the priors' `pitch` conditioning should be for an upload, whose pitch nobody knows.

YIN (de Cheveigne & Kawahara 2002) without the multi-period refinement, on the sound brought to 48 kHz -- three times the
models' rate, because at 16 kHz the dip of the difference function of a bright tone is narrower than one lag and the
first lag under the threshold is then a multiple of the period (specification: tests/pitch_spec.py):

    x = resample(audio, fs_hz, 48000), zero-padded to W + TAU_MAX samples when shorter
    d[t][tau] = sum_{j < W} (x[s + j] - x[s + j + tau])^2, s = t HOP        (csrc/pitch.hip, isi_pitch_difference_f32)
    d'(tau) = d(tau) tau / sum_{k = 1 .. tau} d(k); the first lag in [TAU_MIN, TAU_MAX) under THR, walked down to its
    local minimum, else the argmin; a parabola through the raw d around it gives the period  (isi_pitch_pick_f32)
    a frame is voiced if d'(tau*) < VOICED_AP and its energy exceeds VOICED_E of the clip's largest; the clip's pitch is
    the lower median of the voiced frames' 69 + 12 log2(FS_A / (440 period)), its confidence the voiced share.

`pitch_contour` runs the same two kernels again on windows of about four periods, for a contour fine enough to act on
(GANsynth_pytorch/bend.py).

No CPU path: the audio must live on the GPU."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Tuple, Union

import torch

from interactive_spectrogram_inpainting import _hip
from GANsynth_pytorch.resample import resample

FS_A = 48000
W = 3072
HOP = 768
TAU_MAX = 1920       # 25 Hz
TAU_MIN = 8          # 6 kHz
THR = 0.1
VOICED_AP = 0.2
VOICED_E = 1e-3


class PitchTrack(NamedTuple):
    midi: torch.Tensor            # [B, T] per-frame pitch in MIDI numbers (of unvoiced frames too: see `voiced`)
    aperiodicity: torch.Tensor    # [B, T] d' at the chosen lag
    energy: torch.Tensor          # [B, T] sum of squares of the frame's W samples
    voiced: torch.Tensor          # [B, T] bool
    times_s: torch.Tensor         # [T] centre of each frame's W samples, in seconds


def difference(x: torch.Tensor, w: int = W, hop: int = HOP, tau_max: int = TAU_MAX) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [B, L] float32 on the GPU (unit stride along L, any row stride >= L) -> (d [B, T, tau_max + 1], energy [B, T])."""
    B, L = x.shape
    lib = _hip.lib()
    T = lib.isi_pitch_frames(L, w, hop, tau_max)
    if T < 0:
        raise ValueError(f"a row of {L} samples is shorter than one frame, {w} + {tau_max}")
    d = torch.empty(B, T, tau_max + 1, dtype=torch.float32, device=x.device)
    energy = torch.empty(B, T, dtype=torch.float32, device=x.device)
    x_stride = x.stride(0) if B > 1 else L
    _hip.check(lib.isi_pitch_difference_f32(x.data_ptr(), x_stride, d.data_ptr(), energy.data_ptr(), B, L, w, hop, tau_max,
                                            C.c_void_p(_hip.stream_ptr(x.device))), "isi_pitch_difference_f32")
    return d, energy


def pick(d: torch.Tensor, tau_min: int = TAU_MIN, thr: float = THR) -> Tuple[torch.Tensor, torch.Tensor]:
    """d [.., tau_max + 1] float32, dense, on the GPU -> (period [..] in samples, aperiodicity [..])."""
    lead, n = d.shape[:-1], d.shape[-1]
    period = torch.empty(lead, dtype=torch.float32, device=d.device)
    aperiodicity = torch.empty(lead, dtype=torch.float32, device=d.device)
    _hip.check(_hip.lib().isi_pitch_pick_f32(d.data_ptr(), period.numel(), tau_min, n - 1, thr, period.data_ptr(),
                                             aperiodicity.data_ptr(), C.c_void_p(_hip.stream_ptr(d.device))),
               "isi_pitch_pick_f32")
    return period, aperiodicity


def estimate_pitch(audio: torch.Tensor, fs_hz: int, return_track: bool = False
                   ) -> Union[Tuple[torch.Tensor, torch.Tensor], Tuple[torch.Tensor, torch.Tensor, PitchTrack]]:
    """audio [L] or [B, L] (float32, on the GPU, any row stride) at fs_hz -> (midi, confidence): the pitch in MIDI
    numbers (float32, NaN when no frame is voiced) and the voiced share of the frames, [B] each (0-d for [L]).
    return_track: also the per-frame `PitchTrack`.  A rate the resampler refuses raises its ValueError."""
    _hip.require_gpu(audio, "audio")
    if audio.dtype != torch.float32:
        raise _hip.HipLibraryError(f"audio has dtype {audio.dtype}; expected float32")
    if audio.dim() not in (1, 2) or audio.shape[-1] == 0:
        raise ValueError(f"expected audio [L] or [B, L] with L > 0, got {tuple(audio.shape)}")
    x = resample(audio, fs_hz, FS_A)
    x = x.unsqueeze(0) if x.dim() == 1 else x
    if x.shape[1] < W + TAU_MAX:
        x = torch.nn.functional.pad(x, (0, W + TAU_MAX - x.shape[1]))
    if x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        x = x.contiguous()
    d, energy = difference(x)
    period, aperiodicity = pick(d)
    # the clip: a few operations on [B, T]
    voiced = (aperiodicity < VOICED_AP) & (energy > VOICED_E * energy.amax(1, keepdim=True))
    midi_t = 69.0 + 12.0 * torch.log2(FS_A / (440.0 * period))
    n = voiced.sum(1)
    ordered = torch.where(voiced, midi_t, torch.full_like(midi_t, float("inf"))).sort(1).values    # voiced first, ascending
    median = ordered.gather(1, ((n - 1).clamp(min=0) // 2).unsqueeze(1)).squeeze(1)
    midi = torch.where(n > 0, median, torch.full_like(median, float("nan")))
    confidence = n.to(torch.float32) / voiced.shape[1]
    if audio.dim() == 1:
        midi, confidence = midi[0], confidence[0]
    if not return_track:
        return midi, confidence
    times = (torch.arange(voiced.shape[1], device=x.device, dtype=torch.float32) * HOP + W / 2) / FS_A
    return midi, confidence, PitchTrack(midi_t, aperiodicity, energy, voiced, times)


def pitch_contour(audio: torch.Tensor, fs_hz: int, periods: float = 4.0) -> PitchTrack:
    """The pitch of ONE voiced clip frame by frame, finely enough to act on (GANsynth_pytorch/bend.py): audio [L] or [1, L].
    `estimate_pitch`'s 64 ms frames average a 6 Hz vibrato away; here the clip's pitch gives the period and the same two
    kernels run again on windows of about `periods` periods:
        W = 64 ceil(periods period / 64) clamped to [256, 3072], hop = W / 4,
        lags limited to floor(0.7 period) .. ceil(1.45 period) + 2 (no octave to fall into),
        frame t is timed (t hop + (W + period) / 2) / 48000: the centre of the samples its chosen lag compares.
    The voiced flags follow `estimate_pitch`'s rule.  ValueError when the clip is unvoiced (it has no period)."""
    if audio.dim() == 2 and audio.shape[0] != 1 or audio.dim() not in (1, 2):
        raise ValueError(f"pitch_contour takes one clip, [L] or [1, L]; got {tuple(audio.shape)}")
    midi, _ = estimate_pitch(audio, fs_hz)
    clip = float(midi.reshape(-1)[0])
    if clip != clip:
        raise ValueError("pitch_contour: the clip is unvoiced, it has no period to size the window by")
    period = FS_A / (440.0 * 2.0 ** ((clip - 69.0) / 12.0))
    w = min(max(64 * int(math.ceil(float(periods) * period / 64.0)), 256), 3072)
    hop, tau_min, tau_max = w // 4, max(int(math.floor(0.7 * period)), 1), int(math.ceil(1.45 * period)) + 2
    x = resample(audio, fs_hz, FS_A)
    x = x.unsqueeze(0) if x.dim() == 1 else x
    if x.shape[1] < w + tau_max:
        x = torch.nn.functional.pad(x, (0, w + tau_max - x.shape[1]))
    if x.stride(1) != 1:
        x = x.contiguous()
    d, energy = difference(x, w, hop, tau_max)
    period_t, aperiodicity = pick(d, tau_min)
    voiced = (aperiodicity < VOICED_AP) & (energy > VOICED_E * energy.amax(1, keepdim=True))
    midi_t = 69.0 + 12.0 * torch.log2(FS_A / (440.0 * period_t))
    times = (torch.arange(voiced.shape[1], device=x.device, dtype=torch.float32) * hop + (w + period) / 2.0) / FS_A
    return PitchTrack(midi_t, aperiodicity, energy, voiced, times)
