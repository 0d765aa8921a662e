"""Bend a sound's pitch over time on MI355X: vibrato, glides, pitch flattening -- at the sound's own length.

`transpose` moves a whole sound by one ratio.  Here the pitch follows a curve s(n), in semitones per output sample:
r = 2^(s / 12) is the local rate and phi = exclusive cumsum(r) the time map.  The sound is stretched by the local rate with
the phase-locked vocoder (GANsynth_pytorch/stretch.py: the stretched sound's frame j sits at phi^-1(j hop) of the source),
then read along phi by the time-warped band-limited read isi_warp_resample_f32 (csrc/warp_resample.hip; specification
tests/warp_resample_spec.py): every instant stays where it was, every frequency is multiplied by r.

    warp(audio [L] or [B, L], positions float64 [N] or [1 or B, N], cutoff=None) -> [.., N]
    bend_maps(L, semitones, times_s, fs_hz, hop) -> (r [L], phi [L], frame positions [J]), float64 (`bend` takes them on the host)
    bend(helper, audio, semitones, times_s=None, preserve_formants=False, formant_order=None, pitch=None) -> the input's shape
    vibrato(helper, audio, rate_hz, depth_cents, onset_s=0.0, ramp_s=0.1)
    glide(helper, audio, from_semitones, to_semitones, start_s=0.0, end_s=None)

With `preserve_formants` every stretched frame is corrected by the true envelope at the curve's local rate before the
synthesis (isi_formant_shift_f32, csrc/formant.hip): the pitch follows the curve, the resonances stay.

Not done: a stretch of the curve at rate 1 still passes the vocoder and the ROLLOFF low-pass (the sound there is the
re-synthesis, not the input's bits); one envelope order per call, no envelope taken from another sound; no gradients.  One curve per call: the rows of a batch are bent alike.  No CPU path: the audio must live on the GPU."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from interactive_spectrogram_inpainting import _hip
from GANsynth_pytorch import stretch as _stretch
from GANsynth_pytorch.resample import ROLLOFF, Z

MAX_SEMITONES = 24.0
CUT_MIN = 0.2        # ISI_WARP_CUT_MIN: the kernel's own floor of the cutoff


def warp(audio: torch.Tensor, positions: torch.Tensor, cutoff: Optional[torch.Tensor] = None) -> torch.Tensor:
    """audio [L] or [B, L] (float32, on the GPU, any row stride) read at `positions` (float64, in source samples, [N] or
    [1 or B, N], on the GPU) -> [.., N]: y[n] = sum_m c h(c (p_n - m)) x[m], the resampler's Kaiser-windowed sinc under the
    cutoff c per output (isi_warp_resample_f32).  cutoff (float32, the positions' shape; clamped to [0.2, 1] by the kernel):
    by default ROLLOFF min(1, 1 / local rate), the local rate from the positions' central differences.  The audio is 0
    outside [0, L); a position that is not finite gives 0."""
    _hip.require_gpu(audio, "audio")
    if not positions.is_cuda:
        raise _hip.HipLibraryError(f"positions live on {positions.device}: this package computes only on an MI355X")
    if audio.dtype != torch.float32:
        raise _hip.HipLibraryError(f"audio has dtype {audio.dtype}; expected float32")
    if positions.dtype != torch.float64:
        raise _hip.HipLibraryError(f"positions have dtype {positions.dtype}; expected float64 (a float32 position near sample "
                                   f"60 000 is good to 2^-8 sample only)")
    if positions.device != audio.device:
        raise _hip.HipLibraryError(f"positions live on {positions.device}, audio on {audio.device}")
    if audio.dim() not in (1, 2) or audio.shape[-1] == 0:
        raise ValueError(f"expected audio [L] or [B, L] with L > 0, got {tuple(audio.shape)}")
    x = audio.unsqueeze(0) if audio.dim() == 1 else audio
    pos = positions.unsqueeze(0) if positions.dim() == 1 else positions
    B, L = x.shape
    if pos.dim() != 2 or pos.shape[0] not in (1, B) or pos.shape[1] < 1:
        raise ValueError(f"positions: expected [N] or [1 or {B}, N], got {tuple(positions.shape)}")
    N = pos.shape[1]
    if cutoff is None:
        cut = default_cutoff(pos)
    else:
        _hip.require_gpu(cutoff, "cutoff")
        cut = cutoff.unsqueeze(0) if cutoff.dim() == 1 else cutoff
        if cut.shape != pos.shape or cut.device != x.device:
            raise ValueError(f"cutoff: expected the positions' shape {tuple(pos.shape)} on {x.device}, got {tuple(cutoff.shape)}")
        cut = cut.to(torch.float32)
    if L > 1 and x.stride(1) != 1 or B > 1 and x.stride(0) < L:
        x = x.contiguous()
    pos, cut = pos.contiguous(), cut.contiguous()
    out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    x_stride = x.stride(0) if B > 1 else L
    _hip.check(_hip.lib().isi_warp_resample_f32(x.data_ptr(), x_stride, pos.data_ptr(), cut.data_ptr(), pos.shape[0],
                                                out.data_ptr(), N, B, L, N, C.c_void_p(_hip.stream_ptr(x.device))),
               "isi_warp_resample_f32")
    return out[0] if audio.dim() == 1 else out


def default_cutoff(positions: torch.Tensor) -> torch.Tensor:
    """positions float64 [rows, N] -> float32 [rows, N]: ROLLOFF min(1, 1 / |local rate|), the rate from central differences
    (one-sided at the two ends; 1 for a single position)"""
    N = positions.shape[-1]
    if N == 1:
        rate = torch.ones_like(positions)
    else:
        rate = torch.empty_like(positions)
        rate[..., 1:-1] = (positions[..., 2:] - positions[..., :-2]) * 0.5
        rate[..., 0] = positions[..., 1] - positions[..., 0]
        rate[..., -1] = positions[..., -1] - positions[..., -2]
    cut = ROLLOFF / rate.abs().clamp(min=1.0)
    return torch.nan_to_num(cut, nan=CUT_MIN).to(torch.float32)


def curve(L: int, semitones, times_s=None, fs_hz: int = 16000, device=None) -> torch.Tensor:
    """The curve per output sample, float64 [L] on `device`.  With `times_s` (ascending seconds, one per value): linear in
    semitones between the control points, held outside them.  Without: `semitones` holds one value (a constant) or L values.
    ValueError for a curve that is not finite or leaves +-24 semitones, and for shapes that do not fit."""
    L = int(L)
    if L < 1:
        raise ValueError(f"a curve needs at least one sample, got L = {L}")
    s = torch.as_tensor(semitones, dtype=torch.float64, device=device).reshape(-1)
    if s.numel() == 0:
        raise ValueError("the curve has no value")
    if times_s is None:
        if s.numel() not in (1, L):
            raise ValueError(f"without times_s the curve holds 1 or L = {L} values, got {s.numel()}")
        out = s.expand(L) if s.numel() == 1 else s
    else:
        t = torch.as_tensor(times_s, dtype=torch.float64, device=s.device).reshape(-1)
        if t.numel() != s.numel():
            raise ValueError(f"{s.numel()} values for {t.numel()} times")
        if not bool(torch.isfinite(t).all()) or (t.numel() > 1 and not bool((t[1:] > t[:-1]).all())):
            raise ValueError("times_s must be finite and strictly ascending")
        at = torch.arange(L, dtype=torch.float64, device=s.device) / float(fs_hz)
        if t.numel() == 1:
            out = s.expand(L)
        else:
            i = (torch.searchsorted(t, at, right=True) - 1).clamp(0, t.numel() - 2)
            w = ((at - t[i]) / (t[i + 1] - t[i])).clamp(0.0, 1.0)
            out = s[i] + w * (s[i + 1] - s[i])
    if not bool(torch.isfinite(out).all()) or float(out.abs().max()) > MAX_SEMITONES:
        raise ValueError(f"the curve must be finite and within +-{MAX_SEMITONES:g} semitones")
    return out


def bend_maps(L: int, semitones, times_s=None, fs_hz: int = 16000, hop: int = 64, device=None
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(r, phi, frames), float64 on `device`: the per-sample rate r = 2^(s / 12) of `curve(L, semitones, times_s, fs_hz)`; the
    time map phi = exclusive cumsum(r): output sample n reads the stretched sound at phi[n]; and the source position, in
    frames, of the stretched sound's frame j: phi^-1(j hop) / hop for every j hop < phi(L), by searchsorted and linear
    interpolation."""
    hop = int(hop)
    if hop < 1:
        raise ValueError(f"hop must be positive, got {hop}")
    s = curve(L, semitones, times_s, fs_hz, device)
    r = torch.exp2(s / 12.0)
    phi = torch.cumsum(r, 0) - r
    n_frames = int(math.ceil(float(phi[-1] + r[-1]) / hop))
    v = torch.arange(n_frames, dtype=torch.float64, device=s.device) * hop
    i = (torch.searchsorted(phi, v, right=True) - 1).clamp(0, L - 1)
    frames = (i.to(torch.float64) + (v - phi[i]) / r[i]) / hop
    return r, phi, frames


def frame_rates(r: torch.Tensor, frames: torch.Tensor, n_fft: int, hop: int) -> torch.Tensor:
    """float32 [J]: the rate r at the centre of every stretched frame.  Frame j of the stretched sound sits at source frame
    p = frames[j]; under the helper's framing a frame at p starts n_fft - hop samples before sample p hop, so its centre is
    sample p hop + hop - n_fft / 2 -- rounded to the nearest sample and clamped to [0, L - 1]."""
    centre = torch.round(frames * hop + (hop - n_fft / 2.0)).clamp(0, r.numel() - 1).to(torch.int64)
    return r[centre].to(torch.float32)


@torch.no_grad()
def bend(helper, audio: torch.Tensor, semitones, times_s=None, preserve_formants: bool = False,
         formant_order: Optional[int] = None, pitch: Optional[float] = None) -> torch.Tensor:
    """audio [L] or [B, L] (float32, on the GPU) -> the same shape, its pitch moved by the curve (`curve`: control points
    `semitones` at `times_s`, or one value per sample) at its own length and timing.  The sound, zero-padded so that the far
    side of the last output's support exists, goes through `helper._stft`, `stretch.stft_stretch` along phi^-1 followed by the
    trailing frames at rate 1, the helper's synthesis, and `warp` along phi.  A curve that is zero everywhere returns the
    input itself.
    preserve_formants: between the vocoder and the synthesis every stretched frame passes `stretch.formant_shift` with the
    curve's rate at the frame's centre (`frame_rates`: sample p hop + hop - n_fft / 2 of the source for a frame at source
    position p, clamped to the sound); the trailing frames behind phi(L) take 1 and are copied.  The envelope's order as
    in `stretch.transpose`: `formant_order`, else from `pitch` (a MIDI number), else from `estimate_pitch` of the sound."""
    if audio.dim() not in (1, 2) or audio.shape[-1] == 0:
        raise ValueError(f"expected audio [L] or [B, L] with L > 0, got {tuple(audio.shape)}")
    L = audio.shape[-1]
    N, hop = helper.n_fft, helper.hop_length
    s = curve(L, semitones, times_s, helper.fs_hz, "cpu")          # bad curves are refused before the GPU is asked for
    if not bool(s.any()):
        return audio
    if not preserve_formants and (formant_order is not None or pitch is not None):
        raise ValueError("bend: formant_order and pitch belong to preserve_formants=True")
    order = None
    if preserve_formants and (formant_order is not None or pitch is not None):
        order = _stretch._envelope_order(helper, audio, formant_order, pitch)       # refused before the GPU is asked for
    _hip.require_gpu(audio, "audio")
    if audio.dtype != torch.float32:
        raise _hip.HipLibraryError(f"audio has dtype {audio.dtype}; expected float32")
    # the maps on the host: a device cumsum's order of additions is not fixed from run to run, and phi's last bits decide
    # the fp32 fraction of every position -- the same call would not return the same bits
    r, phi, frames = bend_maps(L, s, None, helper.fs_hz, hop, "cpu")
    dev = audio.device
    x = audio.unsqueeze(0) if audio.dim() == 1 else audio
    cut = (ROLLOFF / r.clamp(min=1.0)).to(torch.float32)
    T, extra = -(-L // hop), N // hop - 1
    tail = int(math.ceil((Z / max(float(cut.min()), CUT_MIN) + 2.0) / hop))       # frames behind phi(L) that the last support reaches into
    T_all = T + extra + tail
    X, got = helper._stft(torch.nn.functional.pad(x, (0, T_all * hop - L)))
    assert got == T_all
    pos = torch.cat([frames.clamp(max=T_all - 1), torch.arange(T, T_all, dtype=torch.float64)]).to(torch.float32)
    Y = _stretch.stft_stretch(X, pos.to(dev), hop)
    if preserve_formants:
        if order is None:
            order = _stretch._envelope_order(helper, audio, None, None)
        rho = torch.cat([frame_rates(r, frames, N, hop), torch.ones(T_all - T, dtype=torch.float32)])
        Y = _stretch.formant_shift(Y, rho.to(dev), order)
    z = _stretch._synthesise(helper, Y, (frames.numel() + tail) * hop)
    out = warp(z, phi.to(dev).unsqueeze(0), cut.to(dev).unsqueeze(0))
    return out[0] if audio.dim() == 1 else out


def vibrato_curve(L: int, fs_hz: int, rate_hz: float, depth_cents: float, onset_s: float = 0.0, ramp_s: float = 0.1,
                  device=None) -> torch.Tensor:
    """depth_cents / 100 * ramp(t) * sin(2 pi rate_hz (t - onset_s)), 0 before the onset; the ramp rises linearly over ramp_s"""
    rate_hz, depth_cents, onset_s, ramp_s = float(rate_hz), float(depth_cents), float(onset_s), float(ramp_s)
    if not (math.isfinite(rate_hz) and rate_hz >= 0.0 and math.isfinite(depth_cents) and math.isfinite(onset_s) and onset_s >= 0.0
            and math.isfinite(ramp_s) and ramp_s >= 0.0):
        raise ValueError(f"vibrato: rate_hz, onset_s and ramp_s must be non-negative and finite, depth_cents finite; got {rate_hz}, "
                         f"{depth_cents}, {onset_s}, {ramp_s}")
    t = torch.arange(int(L), dtype=torch.float64, device=device) / float(fs_hz) - onset_s
    ramp = (t / ramp_s).clamp(0.0, 1.0) if ramp_s > 0.0 else (t >= 0).to(torch.float64)
    return depth_cents / 100.0 * ramp * torch.sin(2.0 * math.pi * rate_hz * t)


def vibrato(helper, audio: torch.Tensor, rate_hz: float, depth_cents: float, onset_s: float = 0.0, ramp_s: float = 0.1,
            preserve_formants: bool = False, formant_order: Optional[int] = None, pitch: Optional[float] = None) -> torch.Tensor:
    """the sound with a vibrato of `rate_hz` and +-`depth_cents` from `onset_s` on, faded in over `ramp_s`; the formant
    arguments are `bend`'s"""
    s = vibrato_curve(audio.shape[-1], helper.fs_hz, rate_hz, depth_cents, onset_s, ramp_s)
    return bend(helper, audio, s, None, preserve_formants, formant_order, pitch)


def glide(helper, audio: torch.Tensor, from_semitones: float, to_semitones: float, start_s: float = 0.0,
          end_s: Optional[float] = None, preserve_formants: bool = False, formant_order: Optional[int] = None,
          pitch: Optional[float] = None) -> torch.Tensor:
    """the sound gliding from `from_semitones` to `to_semitones` (linear in semitones) between start_s and end_s (the end of
    the sound by default), held before and after; the formant arguments are `bend`'s"""
    end_s = audio.shape[-1] / float(helper.fs_hz) if end_s is None else float(end_s)
    start_s = float(start_s)
    if not (math.isfinite(start_s) and math.isfinite(end_s) and 0.0 <= start_s < end_s):
        raise ValueError(f"glide: need 0 <= start_s < end_s, got {start_s} and {end_s}")
    return bend(helper, audio, [float(from_semitones), float(to_semitones)], [start_s, end_s], preserve_formants, formant_order,
                pitch)
