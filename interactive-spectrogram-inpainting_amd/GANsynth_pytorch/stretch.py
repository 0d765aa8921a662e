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
    transpose(helper, audio, semitones, preserve_formants=False, formant_order=None, pitch=None) -> the input's shape

A transposition reads the sound faster or slower, so the whole spectrum moves, resonances included.  With
`preserve_formants` the stretched frames are corrected by the true envelope first (isi_formant_shift_f32, csrc/formant.hip;
specification tests/formant_spec.py): a component that will end at rho f takes the envelope's value
there, and the resonances stay where they were.

    formant_order(fs_hz, f0_hz) -> int, half the pitch period in samples
    formant_shift(Y [B, T, 2F], ratio [T] or [1 or B, T], order, iterations=16, floor_db=80, max_gain_db=40, return_envelope=False)
    spectral_envelope(helper, audio, order=None, pitch=None) -> [.., T, F + 1] in nepers
    shift_formants(helper, audio, semitones, order=None, pitch=None) -> the sound at its own pitch, its formants moved

Not done: transient detection (`keep_attack_s` is the caller's knowledge), per-row envelope orders in a batch (one order
per call), imposing one sound's envelope on another, gradients.  No CPU path: the audio must live on the GPU."""
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


DB = math.log(10.0) / 20.0              # nepers per dB
UNVOICED_ORDER = 32
_TABLES = {}


def formant_order(fs_hz: float, f0_hz: float) -> int:
    """round(0.5 fs / f0) clamped to [4, 256]: half the pitch period in samples, where the Hann lifter reaches zero -- the
    envelope then follows what changes more slowly than the partials' spacing.  ValueError unless both are positive and finite."""
    fs_hz, f0_hz = float(fs_hz), float(f0_hz)
    if not (math.isfinite(fs_hz) and math.isfinite(f0_hz) and fs_hz > 0.0 and f0_hz > 0.0):
        raise ValueError(f"formant_order: fs_hz and f0_hz must be positive and finite, got {fs_hz} and {f0_hz}")
    return int(min(max(round(0.5 * fs_hz / f0_hz), 4), _hip.FORMANT_MAX_ORDER))


def _cos_table(F: int, device) -> torch.Tensor:
    """cos(pi i / F), i < 2F: float64 on the host, rounded once (the entries on the axes are exact)"""
    key = (int(F), str(device))
    if key not in _TABLES:
        c = np.cos(math.pi * np.arange(2 * F) / F)
        c[0], c[F] = 1.0, -1.0
        if F % 2 == 0:
            c[F // 2] = c[3 * F // 2] = 0.0
        _TABLES[key] = torch.from_numpy(c.astype(np.float32)).to(device)
    return _TABLES[key]


def formant_shift(Y: torch.Tensor, ratio: torch.Tensor, order: int, iterations: int = 16, floor_db: float = 80.0,
                  max_gain_db: float = 40.0, return_envelope: bool = False):
    """Y float32 [B, T, 2F] (`stft_stretch`'s layout), ratio float32 [T] or [1 or B, T], both on the GPU -> [B, T, 2F]:
    isi_formant_shift_f32.  Every frame is multiplied by exp(V(rho k) - V(k)), V its true envelope of `order` cepstral
    coefficients after `iterations` passes, the log spectrum floored `floor_db` under the frame's peak and the gain held
    within +-`max_gain_db`; rho is the frame's ratio clamped to [1/4, 4].  A frame whose ratio is 1 or NaN, and a frame that
    is silent or holds a value that is not finite, is returned bit for bit.  return_envelope: also V [B, T, F + 1] in nepers.
    ValueError for shapes and arguments the kernel refuses."""
    _hip.require_gpu(Y, "Y")
    _hip.require_gpu(ratio, "ratio")
    if Y.dtype != torch.float32 or ratio.dtype != torch.float32:
        raise _hip.HipLibraryError(f"Y and ratio must be float32, got {Y.dtype} and {ratio.dtype}")
    if ratio.device != Y.device:
        raise _hip.HipLibraryError(f"ratio lives on {ratio.device}, Y on {Y.device}")
    if ratio.dim() == 1:
        ratio = ratio.unsqueeze(0)
    if Y.dim() != 3 or Y.shape[-1] % 2 or Y.shape[-1] < 4 or Y.shape[0] < 1 or Y.shape[1] < 1:
        raise ValueError(f"Y: expected [B, T, 2F] with F >= 2, got {tuple(Y.shape)}")
    B, T, F = Y.shape[0], Y.shape[1], Y.shape[2] // 2
    if F > _hip.STFT_STRETCH_MAX_F:
        raise ValueError(f"isi_formant_shift_f32 does not take F = {F} (at most {_hip.STFT_STRETCH_MAX_F})")
    if ratio.dim() != 2 or ratio.shape[0] not in (1, B) or ratio.shape[1] != T:
        raise ValueError(f"ratio: expected [T] or [1 or {B}, {T}], got {tuple(ratio.shape)}")
    order, iterations = int(order), int(iterations)
    if not 2 <= order <= min(F, _hip.FORMANT_MAX_ORDER):
        raise ValueError(f"order must lie in 2 .. {min(F, _hip.FORMANT_MAX_ORDER)}, got {order}")
    if not 1 <= iterations <= _hip.FORMANT_MAX_ITERATIONS:
        raise ValueError(f"iterations must lie in 1 .. {_hip.FORMANT_MAX_ITERATIONS}, got {iterations}")
    depth, max_gain = float(floor_db) * DB, float(max_gain_db) * DB
    if not (math.isfinite(depth) and math.isfinite(max_gain) and depth >= 0.0 and max_gain >= 0.0):
        raise ValueError(f"floor_db and max_gain_db must be finite and not negative, got {floor_db} and {max_gain_db}")
    Y, ratio = Y.contiguous(), ratio.contiguous()
    out = torch.empty_like(Y)
    env = torch.empty(B, T, F + 1, dtype=torch.float32, device=Y.device) if return_envelope else None
    _hip.check(_hip.lib().isi_formant_shift_f32(Y.data_ptr(), ratio.data_ptr(), ratio.shape[0], _cos_table(F, Y.device).data_ptr(),
                                                out.data_ptr(), env.data_ptr() if return_envelope else None, B, T, F, order,
                                                iterations, depth, max_gain, C.c_void_p(_hip.stream_ptr(Y.device))),
               "isi_formant_shift_f32")
    return (out, env) if return_envelope else out


def _envelope_order(helper, audio: torch.Tensor, order: Optional[int], pitch: Optional[float]) -> int:
    """the order in this precedence: `order`, `pitch` (a MIDI number), `estimate_pitch` of the sound (the first row of a
    batch that is voiced); 32 for an unvoiced sound.  Never above F of the helper."""
    F = helper.n_fft // 2
    if order is not None:
        order = int(order)
        if not 2 <= order <= min(F, _hip.FORMANT_MAX_ORDER):
            raise ValueError(f"formant order must lie in 2 .. {min(F, _hip.FORMANT_MAX_ORDER)}, got {order}")
        return order
    if pitch is None:
        from GANsynth_pytorch.pitch import estimate_pitch
        midi = estimate_pitch(audio, int(helper.fs_hz))[0].reshape(-1)
        voiced = midi[~torch.isnan(midi)]
        if voiced.numel() == 0:
            return min(UNVOICED_ORDER, F)
        pitch = float(voiced[0])
    pitch = float(pitch)
    if not math.isfinite(pitch):
        raise ValueError(f"pitch must be a finite MIDI number, got {pitch}")
    return min(formant_order(helper.fs_hz, 440.0 * 2.0 ** ((pitch - 69.0) / 12.0)), F)


def _check_audio(audio: torch.Tensor) -> None:
    if audio.dim() not in (1, 2) or audio.shape[-1] == 0:
        raise ValueError(f"expected audio [L] or [B, L] with L > 0, got {tuple(audio.shape)}")
    _hip.require_gpu(audio, "audio")
    if audio.dtype != torch.float32:
        raise _hip.HipLibraryError(f"audio has dtype {audio.dtype}; expected float32")


def _analyse(helper, x: torch.Tensor):
    """x [B, L] -> (X [B, T + extra, 2F], T): the helper's STFT of the sound zero-padded as `time_stretch` pads it"""
    hop = helper.hop_length
    extra, T = helper.n_fft // hop - 1, -(-x.shape[1] // hop)
    X, T_all = helper._stft(torch.nn.functional.pad(x, (0, T * hop - x.shape[1] + extra * hop)))
    assert T_all == T + extra
    return X, T


@torch.no_grad()
def spectral_envelope(helper, audio: torch.Tensor, order: Optional[int] = None, pitch: Optional[float] = None) -> torch.Tensor:
    """audio [L] or [B, L] -> [.., T, F + 1], T = ceil(L / hop): the true envelope of every frame of the helper's STFT in
    nepers (ln of the magnitude), on DFT bins 0 .. F; a silent frame's row is 0.  The order as in `transpose`."""
    _check_audio(audio)
    x = audio.unsqueeze(0) if audio.dim() == 1 else audio
    order = _envelope_order(helper, audio, order, pitch)
    X, T = _analyse(helper, x)
    X = X[:, :T].contiguous()
    env = formant_shift(X, torch.ones(T, dtype=torch.float32, device=X.device), order, return_envelope=True)[1]
    return env[0] if audio.dim() == 1 else env


@torch.no_grad()
def shift_formants(helper, audio: torch.Tensor, semitones: float, order: Optional[int] = None, pitch: Optional[float] = None
                   ) -> torch.Tensor:
    """audio [L] or [B, L] -> the same shape at its own pitch and length, its formants `semitones` higher (lower when
    negative): the helper's STFT, isi_formant_shift_f32 with rho = 2^(-semitones / 12) (the value at f is then taken from
    f / 2^(semitones / 12): the envelope moves up), the helper's synthesis.  0 returns the input itself."""
    semitones = float(semitones)
    if not math.isfinite(semitones):
        raise ValueError(f"semitones must be finite, got {semitones}")
    if semitones == 0.0:
        return audio
    _check_audio(audio)
    x = audio.unsqueeze(0) if audio.dim() == 1 else audio
    order = _envelope_order(helper, audio, order, pitch)
    X, T = _analyse(helper, x)
    ratio = torch.full((X.shape[1],), 2.0 ** (-semitones / 12.0), dtype=torch.float32, device=X.device)
    out = _synthesise(helper, formant_shift(X, ratio, order), T * helper.hop_length)[:, :x.shape[1]].contiguous()
    return out[0] if audio.dim() == 1 else out


@torch.no_grad()
def time_stretch(helper, audio: torch.Tensor, factor: float, keep_attack_s: float = 0.0, keep_release_s: float = 0.0,
                 _formant=None) -> torch.Tensor:
    """audio [L] or [B, L] (float32, on the GPU) -> [.., T_out hop] with T = ceil(L / hop), T_out = max(1, round(T factor)):
    the sound `factor` times as long at its own pitch.  The first `keep_attack_s` and the last `keep_release_s` seconds keep
    their own rate.  The STFT is taken of the audio zero-padded by n_fft / hop - 1 hops, as `to_audio_spliced` does; those
    trailing frames follow the stretched ones at rate 1, so that the last samples meet complete overlap sums.  factor == 1
    re-synthesises the sound from its own frames (the DC bin is dropped, nothing else).  `_formant` = (rho, order) is
    `transpose`'s hook: the stretched frames, the trailing ones included, pass `formant_shift` at that ratio."""
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
    if _formant is not None:                             # (rho, order): `transpose` corrects the stretched frames
        rho, order = _formant
        Y = formant_shift(Y, torch.full((Y.shape[1],), rho, dtype=torch.float32, device=Y.device), order)
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
def transpose(helper, audio: torch.Tensor, semitones: float, preserve_formants: bool = False,
              formant_order: Optional[int] = None, pitch: Optional[float] = None) -> torch.Tensor:
    """audio [L] or [B, L] -> the same shape, `semitones` higher (lower when negative) at its own length: `time_stretch` by
    num / den = `transpose_ratio(semitones)`, then `resample(y, num, den)`, trimmed or zero-padded to L.  0 semitones
    returns the input itself.
    preserve_formants: the stretched frames pass `formant_shift` with rho = num / den between the vocoder and the synthesis,
    so that the resonances stay where they were.  The envelope's order, in this precedence: `formant_order`; `formant_order
    (fs, f0)` of `pitch`, the source's MIDI number; of `estimate_pitch` of the sound (32 when it is unvoiced).  One order per
    call: a batch takes its first voiced row's."""
    num, den, _ = transpose_ratio(semitones)
    if num == den:
        return audio
    hook = None
    if preserve_formants:
        if audio.dim() not in (1, 2) or audio.shape[-1] == 0:
            raise ValueError(f"expected audio [L] or [B, L] with L > 0, got {tuple(audio.shape)}")
        hook = (num / den, _envelope_order(helper, audio, formant_order, pitch))
    elif formant_order is not None or pitch is not None:
        raise ValueError("transpose: formant_order and pitch belong to preserve_formants=True")
    y = time_stretch(helper, audio, num / den) if hook is None else time_stretch(helper, audio, num / den, _formant=hook)
    z = _resample.resample(y, num, den)
    L = audio.shape[-1]
    if z.shape[-1] < L:
        z = torch.nn.functional.pad(z, (0, L - z.shape[-1]))
    return z[..., :L].contiguous()
