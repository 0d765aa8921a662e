"""Band-limited sample-rate conversion on MI355X: brings an upload at the recorder's rate (44.1 or 48 kHz in practice) to
the models' rate, and audio output to a requested one.

The reference's /analyze-audio hands the uploaded file to `spectrograms_helper.from_wavfile(path, duration_n=...)`, which
resamples with sox / torchaudio and scales the duration by FS_HZ / original_fs_hz (reference flask_server.py:557-568,
624-667).  Those packages are absent; the arithmetic is this project's own (specification: tests/resample_spec.py,
DESIGN.md "Sample-rate conversion"): a polyphase Kaiser-windowed sinc with the "kaiser best" constants,

    g = gcd(fs_in, fs_out), orig = fs_in / g, new = fs_out / g, f0 = ROLLOFF min(orig, new)
    width = ceil(Z orig / f0), taps = 2 width + orig, N_out = ceil(L new / orig)
    h[r][i] = (f0 / orig) sinc(t) I0(BETA sqrt(1 - (t / Z)^2)) / I0(BETA),  t = clip(f0 ((i - width) / orig - r / new), -Z, Z)
    y[q new + r] = sum_i h[r][i] x[q orig + i - width],  x = 0 outside [0, L)

The table is evaluated in float64 on the host and rounded once to fp32; the sums are the direct-form FIR kernel of
csrc/resample.hip (isi_resample_f32).  No CPU path: the audio must live on the GPU."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Tuple

import numpy as np
import torch

from interactive_spectrogram_inpainting import _hip

Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492

_tables: Dict[Tuple[int, int, torch.device], torch.Tensor] = {}


def geometry(fs_in: int, fs_out: int) -> Tuple[int, int, int, int]:
    """(orig, new, width, taps) of a conversion, from the library (isi_resample_geometry, host only).  ValueError for a
    rate <= 0 and for a ratio beyond the kernel's caps (taps <= 16384, new * taps <= 2^22), naming the reduced ratio."""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in <= 0 or fs_out <= 0 or max(fs_in, fs_out) >= 2 ** 31:
        raise ValueError(f"sampling rates must be positive 32-bit integers, got {fs_in} -> {fs_out} Hz")
    out = [C.c_int(0) for _ in range(4)]
    rc = _hip.lib().isi_resample_geometry(fs_in, fs_out, *[C.byref(v) for v in out])
    orig, new, width, taps = (v.value for v in out)
    if rc != 0:
        g = math.gcd(fs_in, fs_out)
        raise ValueError(f"cannot resample {fs_in} Hz to {fs_out} Hz: the reduced ratio {fs_out // g}/{fs_in // g} needs "
                         f"{taps} taps in {new} phases, beyond the kernel's caps (16384 taps, 2^22 coefficients)")
    return orig, new, width, taps


def resample_table(fs_in: int, fs_out: int) -> np.ndarray:
    """The coefficients h [new, taps] in float64, on the host (evaluated once per ratio, like the DFT bases)."""
    orig, new, width, taps = geometry(fs_in, fs_out)
    f0 = ROLLOFF * min(orig, new)
    j = np.arange(taps, dtype=np.float64) - width
    r = np.arange(new, dtype=np.float64)
    t = np.clip(f0 * (j[None, :] / orig - r[:, None] / new), -Z, Z)
    window = np.i0(BETA * np.sqrt(1.0 - (t / Z) ** 2)) / np.i0(BETA)
    return (f0 / orig) * np.sinc(t) * window


def _device_table(fs_in: int, fs_out: int, orig: int, new: int, device: torch.device) -> torch.Tensor:
    key = (orig, new, device)
    table = _tables.get(key)
    if table is None:
        h = resample_table(fs_in, fs_out).astype(np.float32)               # the one rounding
        table = torch.from_numpy(np.ascontiguousarray(h.T)).to(device)     # tap-major [taps, new]
        _tables[key] = table
    return table


def _run(audio: torch.Tensor, orig: int, new: int, width: int, table: torch.Tensor) -> torch.Tensor:
    """[B, L] (unit stride along L, any row stride >= L) -> [B, N_out] with the given tap-major device table."""
    B, L = audio.shape
    lib = _hip.lib()
    n_out = lib.isi_resample_out_len(L, orig, new)
    out = torch.empty(B, n_out, dtype=torch.float32, device=audio.device)
    if B == 0 or L == 0:
        return out
    x_stride = audio.stride(0) if B > 1 else L
    _hip.check(lib.isi_resample_f32(audio.data_ptr(), x_stride, out.data_ptr(), n_out, B, L, orig, new, width,
                                    table.data_ptr(), C.c_void_p(_hip.stream_ptr(audio.device))), "isi_resample_f32")
    return out


def resample(audio: torch.Tensor, fs_in: int, fs_out: int) -> torch.Tensor:
    """audio [L] or [B, L] (float32, on the GPU, any row stride) at fs_in -> [.., ceil(L new / orig)] at fs_out.
    fs_in == fs_out is the identity: no launch, the input is returned."""
    _hip.require_gpu(audio, "audio")
    if audio.dtype != torch.float32:
        raise _hip.HipLibraryError(f"audio has dtype {audio.dtype}; expected float32")
    if audio.dim() not in (1, 2):
        raise ValueError(f"expected audio [L] or [B, L], got {tuple(audio.shape)}")
    if int(fs_in) == int(fs_out):
        return audio
    orig, new, width, _ = geometry(fs_in, fs_out)
    x = audio.unsqueeze(0) if audio.dim() == 1 else audio
    if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        x = x.contiguous()
    out = _run(x, orig, new, width, _device_table(int(fs_in), int(fs_out), orig, new, x.device))
    return out[0] if audio.dim() == 1 else out
