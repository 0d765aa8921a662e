"""Specification of the pitch estimator (GANsynth_pytorch/pitch.py, csrc/pitch.hip), in NumPy float64 (DESIGN.md
section 6d).  YIN (de Cheveigne & Kawahara, JASA 111 (4), 2002) without its multi-period refinement, run at three times
the models' rate: with partials up to 7.6 kHz the dip of the difference function is narrower than one lag at 16 kHz,
integer lags miss it and the first lag under the threshold is a multiple of the period; at 48 kHz it spans about 3 lags.

    x = resample(audio, fs_hz, FS_A) (tests/resample_spec.py), zero-padded to W + TAU_MAX samples when shorter
    T = (L - W - TAU_MAX) // HOP + 1 frames, frame t starts at s = t HOP
    d[t][tau] = sum_{j < W} (x[s + j] - x[s + j + tau])^2 for tau in [0, TAU_MAX],  e[t] = sum_{j < W} x[s + j]^2
    cs(tau) = sum_{k = 1 .. tau} d(k),  d'(0) = 1,  d'(tau) = d(tau) tau / cs(tau),  d' = 1 where cs = 0
    tau* = the smallest tau in [TAU_MIN, TAU_MAX) with d'(tau) < THR, then tau -> tau + 1 while tau + 1 < TAU_MAX and
           d'(tau + 1) < d'(tau); with no lag under the threshold the argmin of d' over [TAU_MIN, TAU_MAX), lowest on ties
    aperiodicity = d'(tau*)
    period = tau* + (a - c) / (2 v) with a, b, c = d(tau* - 1), d(tau*), d(tau* + 1), v = a - 2 b + c, if v > 0; else tau*
    voiced(t) = aperiodicity < VOICED_AP and e[t] > VOICED_E max_t e
    midi_t = 69 + 12 log2(FS_A / (440 period_t)),  pitch = lower median of the voiced midi_t (sorted[(n - 1) // 2]),
    confidence = the voiced share; with no voiced frame pitch = NaN, confidence = 0

`difference` is the definition.  `difference_by_correlation` is the same quantity as E_a + E_tau - 2 corr in float64 (the
subtraction costs 2^-53 E / d there, nothing at the sizes of the tests -- in fp32 it would cost 2^-24 E / d, which is why
the kernel takes the direct form): it is what the clip-level functions use, being a hundred times quicker in NumPy.
Imports nothing from the product."""
import numpy as np

import resample_spec

FS_A = 48000
W = 3072
HOP = 768
TAU_MAX = 1920       # 25 Hz
TAU_MIN = 8          # 6 kHz
THR = 0.1
VOICED_AP = 0.2
VOICED_E = 1e-3


def frames(L: int, w: int = W, hop: int = HOP, tau_max: int = TAU_MAX) -> int:
    return (L - w - tau_max) // hop + 1


def analysis_signal(audio, fs_hz: int, w: int = W, tau_max: int = TAU_MAX) -> np.ndarray:
    """[.., L] at fs_hz -> float64 [.., max(L', w + tau_max)] at FS_A."""
    x = resample_spec.resample(np.asarray(audio, dtype=np.float64), int(fs_hz), FS_A)
    short = w + tau_max - x.shape[-1]
    if short > 0:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (short,))], axis=-1)
    return x


def difference(x, w: int = W, hop: int = HOP, tau_max: int = TAU_MAX):
    """The definition: x [L] -> (d [T, tau_max + 1], e [T]) in float64."""
    x = np.asarray(x, dtype=np.float64)
    T = frames(x.shape[-1], w, hop, tau_max)
    d = np.empty((T, tau_max + 1))
    e = np.empty(T)
    for t in range(T):
        seg = x[t * hop:t * hop + w + tau_max]
        lagged = np.lib.stride_tricks.sliding_window_view(seg, w)        # [tau_max + 1, w]: lagged[tau][j] = seg[j + tau]
        d[t] = ((seg[None, :w] - lagged) ** 2).sum(1)
        e[t] = (seg[:w] ** 2).sum()
    return d, e


def difference_by_correlation(x, w: int = W, hop: int = HOP, tau_max: int = TAU_MAX):
    """d = E_a + E_tau - 2 corr in float64, clamped at 0: equal to `difference` to about 2^-50 of the frame energy."""
    x = np.asarray(x, dtype=np.float64)
    T = frames(x.shape[-1], w, hop, tau_max)
    d = np.empty((T, tau_max + 1))
    e = np.empty(T)
    sq = np.concatenate([[0.0], np.cumsum(x * x)])
    taus = np.arange(tau_max + 1)
    for t in range(T):
        s = t * hop
        seg = x[s:s + w + tau_max]
        corr = np.correlate(seg, seg[:w], mode="valid")                  # corr[tau] = sum_j seg[j] seg[j + tau]
        e_tau = sq[s + taus + w] - sq[s + taus]
        e[t] = (seg[:w] ** 2).sum()
        d[t] = np.maximum(e[t] + e_tau - 2.0 * corr, 0.0)
        d[t, 0] = 0.0
    return d, e


def normalise(d) -> np.ndarray:
    """d [.., n] -> d' [.., n]."""
    d = np.asarray(d, dtype=np.float64)
    cs = np.cumsum(d[..., 1:], axis=-1)
    tau = np.arange(1, d.shape[-1], dtype=np.float64)
    dp = np.ones_like(d)
    np.divide(d[..., 1:] * tau, cs, out=dp[..., 1:], where=cs > 0)
    return dp


def pick(d, tau_min: int = TAU_MIN, tau_max: int = TAU_MAX, thr: float = THR):
    """d [T, tau_max + 1] -> (tau [T] int, period [T], aperiodicity [T], margin [T]).  margin: the smallest relative gap
    |p - q| / max(|p|, |q|) over the comparisons the choice of tau made on that frame -- the threshold against every lag it
    passed (the chosen one included), every step of the descent (the one that stopped it included) and, in the fallback,
    the best against the runner-up.  An evaluation whose d' carries a relative error below half the margin makes the
    same choice."""
    d = np.asarray(d, dtype=np.float64)
    dp = normalise(d)
    T = d.shape[0]
    tau = np.empty(T, dtype=np.int64)
    period = np.empty(T)
    margin = np.empty(T)

    def gap(p, q):
        m = max(abs(p), abs(q))
        return abs(p - q) / m if m > 0 else 0.0
    for t in range(T):
        row = dp[t]
        under = np.flatnonzero(row[tau_min:tau_max] < thr)
        if under.size:
            k = tau_min + int(under[0])
            m = min(gap(v, thr) for v in row[tau_min:k + 1])
            while k + 1 < tau_max:
                m = min(m, gap(row[k + 1], row[k]))
                if not row[k + 1] < row[k]:
                    break
                k += 1
        else:
            k = tau_min + int(np.argmin(row[tau_min:tau_max]))           # argmin: the first of equal minima
            others = np.delete(row[tau_min:tau_max], k - tau_min)
            m = min(min(gap(v, thr) for v in row[tau_min:tau_max]), gap(others.min(), row[k]))
        a, b, c = d[t, k - 1], d[t, k], d[t, k + 1]
        v = a - 2.0 * b + c
        tau[t], margin[t] = k, m
        period[t] = k + (a - c) / (2.0 * v) if v > 0 else float(k)
    return tau, period, dp[np.arange(T), tau], margin


def clip(period, aperiodicity, energy, fs_a: float = FS_A, voiced_ap: float = VOICED_AP, voiced_e: float = VOICED_E):
    """Per-frame results of one clip -> (pitch, confidence, midi [T], voiced [T])."""
    period, aperiodicity, energy = (np.asarray(v, dtype=np.float64) for v in (period, aperiodicity, energy))
    voiced = (aperiodicity < voiced_ap) & (energy > voiced_e * energy.max())
    midi = 69.0 + 12.0 * np.log2(fs_a / (440.0 * period))
    n = int(voiced.sum())
    if n == 0:
        return float("nan"), 0.0, midi, voiced
    return float(np.sort(midi[voiced])[(n - 1) // 2]), n / voiced.size, midi, voiced


def estimate(audio, fs_hz: int, direct: bool = False):
    """One clip [L] at fs_hz -> (pitch in MIDI numbers or NaN, confidence), at the constants above."""
    x = analysis_signal(audio, fs_hz)
    d, e = (difference if direct else difference_by_correlation)(x)
    _, period, ap, _ = pick(d)
    return clip(period, ap, e)[:2]
