"""Specification of the band-limited sample-rate converter (GANsynth_pytorch/resample.py, csrc/resample.hip), in NumPy
float64.  The sox / torchaudio resamplers the reference leans on (`from_wavfile`, reference flask_server.py:557-568,
624-667) are absent, so this text -- not those packages -- fixes the arithmetic ("Sample-rate conversion").
A Kaiser-windowed sinc with the widely published "kaiser best" constants, evaluated as a polyphase FIR:

    g = gcd(fs_in, fs_out), orig = fs_in / g, new = fs_out / g
    f0 = ROLLOFF min(orig, new), width = ceil(Z orig / f0), taps = 2 width + orig
    h[r][i] = (f0 / orig) sinc(t) I0(BETA sqrt(1 - (t / Z)^2)) / I0(BETA),  t = clip(f0 ((i - width) / orig - r / new), -Z, Z)
    y[q new + r] = sum_i h[r][i] x[q orig + i - width]   (x = 0 outside [0, L)),   N_out = ceil(L new / orig)

The table is evaluated in float64 and rounded once to fp32; every tap is multiplied (the clamped ones are about 1e-23).
Imports nothing from the product."""
import functools
import math

import numpy as np

Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492


def geometry(fs_in: int, fs_out: int):
    """(orig, new, width, taps)."""
    g = math.gcd(fs_in, fs_out)
    orig, new = fs_in // g, fs_out // g
    f0 = ROLLOFF * min(orig, new)
    width = math.ceil(Z * orig / f0)
    return orig, new, width, 2 * width + orig


def out_len(L: int, orig: int, new: int) -> int:
    return -(-L * new // orig)


def i0(x: np.ndarray) -> np.ndarray:
    """Modified Bessel function of the first kind, order 0: the power series sum_k ((x / 2)^k / k!)^2 (positive terms,
    so the float64 sum is good to a few ulp; 60 terms leave less than 1e-30 of the sum at x = BETA)."""
    x = np.asarray(x, dtype=np.float64)
    term = np.ones_like(x)
    total = np.ones_like(x)
    for k in range(1, 60):
        term = term * (x / 2.0) / k
        total = total + term * term
    return total


def sinc(t: np.ndarray) -> np.ndarray:
    t = np.asarray(t, dtype=np.float64)
    y = np.pi * np.where(t == 0.0, 1.0, t)
    return np.where(t == 0.0, 1.0, np.sin(y) / y)


@functools.lru_cache(maxsize=None)
def table64(fs_in: int, fs_out: int) -> np.ndarray:
    """h [new, taps] in float64."""
    orig, new, width, taps = geometry(fs_in, fs_out)
    f0 = ROLLOFF * min(orig, new)
    j = np.arange(taps, dtype=np.float64) - width
    r = np.arange(new, dtype=np.float64)
    t = np.clip(f0 * (j[None, :] / orig - r[:, None] / new), -Z, Z)
    h = (f0 / orig) * sinc(t) * i0(BETA * np.sqrt(1.0 - (t / Z) ** 2)) / i0(np.float64(BETA))
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def table32(fs_in: int, fs_out: int) -> np.ndarray:
    """The table the kernel is given: h rounded once to fp32, [new, taps]."""
    h = table64(fs_in, fs_out).astype(np.float32)
    h.setflags(write=False)
    return h


def resample(x: np.ndarray, fs_in: int, fs_out: int, with_abs: bool = False):
    """y [.., N_out] in float64 from x [.., L]: the fp32-rounded table, float64 products and sums.  with_abs: also
    sum_i |h[r][i] x[..]| per output (the scale of the rounding bound of an fp32 evaluation)."""
    x = np.asarray(x, dtype=np.float64)
    if fs_in == fs_out:
        return (x, np.abs(x)) if with_abs else x
    orig, new, width, taps = geometry(fs_in, fs_out)
    h = table32(fs_in, fs_out).astype(np.float64)
    L = x.shape[-1]
    n_out = out_len(L, orig, new)
    n = np.arange(n_out)
    q, r = n // new, n % new
    n_pad = (int(q[-1]) if n_out else 0) * orig + taps
    xp = np.zeros(x.shape[:-1] + (max(n_pad, width + L),), dtype=np.float64)
    xp[..., width:width + L] = x                                  # xp[k] = x[k - width]
    idx = q[:, None] * orig + np.arange(taps)[None, :]            # [N_out, taps]
    prod = h[r][None] * xp.reshape(-1, xp.shape[-1])[:, idx]      # [rows, N_out, taps]
    y = prod.sum(-1).reshape(x.shape[:-1] + (n_out,))
    if with_abs:
        return y, np.abs(prod).sum(-1).reshape(x.shape[:-1] + (n_out,))
    return y
