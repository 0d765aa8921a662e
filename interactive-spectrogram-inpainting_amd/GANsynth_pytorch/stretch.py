"""Time stretch and transposition of a sound on MI355X: a phase vocoder with identity phase locking.

Everything else in the project takes an upload's length and pitch as given.  Here the sound's STFT (the helper's own: DC
dropped, hop dividing n_fft) is re-timed along a list of source positions, one per output frame, by isi_stft_stretch_f32
(csrc/stft_stretch.hip; specification: tests/stft_stretch_spec.py): magnitudes are interpolated, every
bin's phase follows the nearest spectral peak of its source frame and keeps the source's phase difference to it, so that
the partials of an attack stay aligned.  A transposition is a stretch by num / den followed by the band-limited resampler
(GANsynth_pytorch/resample.py) reading the result den / num times as fast.

    stretch_positions(n_frames, factor=None, n_out=None, keep_head=0, keep_tail=0) -> float32 [n_out] (host)
    stft_stretch(X [B, T, 2F], positions [T_out] or [1 or B, T_out], hop) -> [B, T_out, 2F]
    time_stretch(helper, audio [L] or [B, L], factor, keep_attack_s=0.0, keep_release_s=0.0) -> [.., T_out hop]
    transpose_ratio(semitones, max_denominator=512) -> (num, den, error in cents)
    transpose(helper, audio, semitones) -> the input's shape

Not done: transient detection (`keep_attack_s` is the caller's knowledge), formant preservation (a transposed voice moves
its formants along), gradients.  No CPU path: the audio must live on the GPU."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np
import torch

from interactive_spectrogram_inpainting import _hip
from GANsynth_pytorch import resample as _resample


def stretch_positions(n_frames: int, factor: Optional[float] = None, n_out: Optional[int] = None, keep_head: int = 0,
                      keep_tail: int = 0) -> torch.Tensor:
    """The source position of every output frame: float32 [n_out] on the host, evaluated in float64 and rounded once.

    n_out = max(1, round(n_frames * factor)) unless given.  The first `keep_head` and the last `keep_tail` source frames
    are kept at rate 1 (an attack, a release); the n_frames - keep_head - keep_tail frames between them are spread
    uniformly over the output frames that remain.  factor == 1 gives 0 .. n_frames - 1 exactly.  ValueError for a
    factor that is not positive and finite, and for a head plus tail that does not fit into both lengths."""
    n_frames, keep_head, keep_tail = int(n_frames), int(keep_head), int(keep_tail)
    if n_frames < 1 or keep_head < 0 or keep_tail < 0:
        raise ValueError(f"stretch_positions: n_frames must be at least 1 and the kept frames non-negative, got {n_frames}, "
                         f"{keep_head}, {keep_tail}")
    if (factor is None) == (n_out is None):
        raise ValueError("stretch_positions: give exactly one of factor and n_out")
    if n_out is None:
        factor = float(factor)
        if not (math.isfinite(factor) and factor > 0.0):
            raise ValueError(f"stretch_positions: factor must be positive and finite, got {factor}")
        n_out = max(1, int(round(n_frames * factor)))
    n_out = int(n_out)
    if n_out < 1:
        raise ValueError(f"stretch_positions: n_out must be at least 1, got {n_out}")
    mid_in, mid_out = n_frames - keep_head - keep_tail, n_out - keep_head - keep_tail
    if mid_in < 0 or mid_out < 0 or (mid_in > 0) != (mid_out > 0):
        raise ValueError(f"stretch_positions: {keep_head} + {keep_tail} kept frames do not fit into {n_frames} source and "
                         f"{n_out} output frames with a stretched part between them")
    middle = keep_head + np.arange(mid_out, dtype=np.float64) * (mid_in / max(mid_out, 1))
    p = np.concatenate([np.arange(keep_head, dtype=np.float64), middle,
                        n_frames - keep_tail + np.arange(keep_tail, dtype=np.float64)])
    return torch.from_numpy(p.astype(np.float32))


def stft_stretch(X: torch.Tensor, positions: torch.Tensor, hop: int) -> torch.Tensor:
    """X float32 [B, T, 2F] (real block | imaginary block, DC dropped), positions float32 [T_out] or [1 or B, T_out] in
    source frames, both on the GPU -> [B, T_out, 2F]: isi_stft_stretch_f32.  A leading run of positions p, p + 1, ... on
    whole frames returns those frames bit for bit.  ValueError for shapes the kernel refuses."""
    _hip.require_gpu(X, "X")
    _hip.require_gpu(positions, "positions")
    if X.dtype != torch.float32 or positions.dtype != torch.float32:
        raise _hip.HipLibraryError(f"X and positions must be float32, got {X.dtype} and {positions.dtype}")
    if positions.device != X.device:
        raise _hip.HipLibraryError(f"positions live on {positions.device}, X on {X.device}")
    if positions.dim() == 1:
        positions = positions.unsqueeze(0)
    if X.dim() != 3 or X.shape[-1] % 2 or X.shape[-1] < 2 or X.shape[0] < 1 or X.shape[1] < 2:
        raise ValueError(f"X: expected [B, T >= 2, 2F], got {tuple(X.shape)}")
    B, T, F = X.shape[0], X.shape[1], X.shape[2] // 2
    if positions.dim() != 2 or positions.shape[0] not in (1, B) or positions.shape[1] < 1:
        raise ValueError(f"positions: expected [T_out] or [1 or {B}, T_out], got {tuple(positions.shape)}")
    hop = int(hop)
    if hop < 1 or (2 * F) % hop:
        raise ValueError(f"hop {hop} does not divide n_fft = {2 * F}")
    X, positions = X.contiguous(), positions.contiguous()
    T_out = positions.shape[1]
    lib = _hip.lib()
    need = lib.isi_stft_stretch_workspace_bytes(B, T, F)
    if need == 0:
        raise ValueError(f"isi_stft_stretch_f32 does not take B = {B}, T = {T}, F = {F}")
    workspace = torch.empty(need // 4, dtype=torch.float32, device=X.device)
    out = torch.empty(B, T_out, 2 * F, dtype=torch.float32, device=X.device)
    _hip.check(lib.isi_stft_stretch_f32(X.data_ptr(), positions.data_ptr(), positions.shape[0], out.data_ptr(),
                                        workspace.data_ptr(), need, B, T, T_out, F, hop,
                                        C.c_void_p(_hip.stream_ptr(X.device))), "isi_stft_stretch_f32")
    return out


def _seconds_to_frames(helper, seconds: float, what: str) -> int:
    seconds = float(seconds)
    if not (math.isfinite(seconds) and seconds >= 0.0):
        raise ValueError(f"{what} must be a non-negative number of seconds, got {seconds}")
    return int(math.ceil(seconds * helper.fs_hz / helper.hop_length))


@torch.no_grad()
def time_stretch(helper, audio: torch.Tensor, factor: float, keep_attack_s: float = 0.0, keep_release_s: float = 0.0
                 ) -> torch.Tensor:
    """audio [L] or [B, L] (float32, on the GPU) -> [.., T_out hop] with T = ceil(L / hop), T_out = max(1, round(T factor)):
    the sound `factor` times as long at its own pitch.  The first `keep_attack_s` and the last `keep_release_s` seconds keep
    their own rate.  The STFT is taken of the audio zero-padded by n_fft / hop - 1 hops, as `to_audio_spliced` does; those
    trailing frames follow the stretched ones at rate 1, so that the last samples meet complete overlap sums.  factor == 1
    re-synthesises the sound from its own frames (the DC bin is dropped, nothing else)."""
    if audio.dim() not in (1, 2) or audio.shape[-1] == 0:
        raise ValueError(f"expected audio [L] or [B, L] with L > 0, got {tuple(audio.shape)}")
    x = audio.unsqueeze(0) if audio.dim() == 1 else audio
    N, hop = helper.n_fft, helper.hop_length
    extra = N // hop - 1
    T = -(-x.shape[1] // hop)
    head, tail = _seconds_to_frames(helper, keep_attack_s, "keep_attack_s"), _seconds_to_frames(helper, keep_release_s, "keep_release_s")
    pos = stretch_positions(T, factor=factor, keep_head=head, keep_tail=tail)      # a bad argument is refused before the GPU is asked for
    _hip.require_gpu(audio, "audio")
    if audio.dtype != torch.float32:
        raise _hip.HipLibraryError(f"audio has dtype {audio.dtype}; expected float32")
    T_out = pos.numel()
    pos = torch.cat([pos, torch.arange(T, T + extra, dtype=torch.float32)])
    X, T_all = helper._stft(torch.nn.functional.pad(x, (0, T * hop - x.shape[1] + extra * hop)))
    assert T_all == T + extra
    if T_all < 2:                                        # hop == n_fft and a single frame: nothing to advance along
        raise ValueError("time_stretch needs at least two frames")
    Y = stft_stretch(X, pos.to(x.device), hop)
    out = _synthesise(helper, Y, T_out * hop)
    return out[0] if audio.dim() == 1 else out


def _synthesise(helper, Y: torch.Tensor, n_out: int) -> torch.Tensor:
    """STFT frames [B, T_all, 2F] -> audio [B, n_out]: the helper's inverse GEMM and overlap-add"""
    from interactive_spectrogram_inpainting.priors import _ops as gemm
    c = helper._build(Y.device)
    B, T_all = Y.shape[0], Y.shape[1]
    frames = gemm.linear(Y, c["istft_w"], None, helper.n_fft)
    out = torch.empty(B, n_out, dtype=torch.float32, device=Y.device)
    _hip.check(_hip.lib().isi_overlap_add_f32(frames.data_ptr(), out.data_ptr(), B, T_all, helper.n_fft, helper.hop_length,
                                              helper.n_fft - helper.hop_length, n_out, C.c_void_p(_hip.stream_ptr(Y.device))),
               "isi_overlap_add_f32")
    return out


def transpose_ratio(semitones: float, max_denominator: int = 512) -> Tuple[int, int, float]:
    """(num, den, error in cents): the best rational num / den for 2^(semitones / 12) with a denominator of at most
    `max_denominator` that the resampler's geometry accepts for the conversion num -> den; the denominator is lowered until
    it does.  `semitones` may be fractional.  ValueError when it is not finite or no ratio is accepted."""
    semitones = float(semitones)
    if not math.isfinite(semitones):
        raise ValueError(f"semitones must be finite, got {semitones}")
    target = 2.0 ** (semitones / 12.0)
    limit = int(max_denominator)
    while limit >= 1:
        r = Fraction(target).limit_denominator(limit)
        if r.numerator >= 1:
            try:
                _resample.geometry(r.numerator, r.denominator)
                return r.numerator, r.denominator, 1200.0 * math.log2((r.numerator / r.denominator) / target)
            except ValueError:
                pass
        limit = min(limit - 1, r.denominator - 1)
    raise ValueError(f"no ratio for {semitones} semitones that the resampler accepts")


@torch.no_grad()
def transpose(helper, audio: torch.Tensor, semitones: float) -> torch.Tensor:
    """audio [L] or [B, L] -> the same shape, `semitones` higher (lower when negative) at its own length: `time_stretch` by
    num / den = `transpose_ratio(semitones)`, then `resample(y, num, den)`, trimmed or zero-padded to L.  0 semitones
    returns the input itself."""
    num, den, _ = transpose_ratio(semitones)
    if num == den:
        return audio
    y = time_stretch(helper, audio, num / den)
    z = _resample.resample(y, num, den)
    L = audio.shape[-1]
    if z.shape[-1] < L:
        z = torch.nn.functional.pad(z, (0, L - z.shape[-1]))
    return z[..., :L].contiguous()
