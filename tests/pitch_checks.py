"""What tests/test_pitch_gpu.py compares the pitch kernels with, kept apart from it so that tests/test_pitch_host.py can
show -- without a GPU -- that each comparison rejects a planted fault.  Signals and bounds only; imports nothing from
the product.

The difference function.  With u = 2^-24 and terms p_j = (x[s+j] - x[s+j+tau])^2 >= 0 of float64 sum d64:
  the subtraction is rounded once, fl(a - b) = (a - b)(1 + e1), |e1| <= u, so its square is p_j (1 + e1)^2;
  fma(df, df, acc) rounds df df + acc once: after W steps every term has gone through at most W roundings, in
  whatever order the steps are taken, so |d - d64| <= ((1 + u)^(W + 2) - 1) d64 <= (W + 4) u d64
  (the terms are non-negative: no cancellation; (1 + u)^(W + 2) - 1 < (W + 4) u for every W below 2^20).
The same bound holds for the energy (W squares, no subtraction).

The pick.  The kernel's d' = d tau / cs has an fp32 prefix sum cs of at most tau_max non-negative terms: relative error
below (tau_max + 2) u in any order, the multiplication and the division included.  A frame is CERTIFIED when every
comparison the float64 choice made has a relative gap above 4 (tau_max + 2) u (pitch_spec.pick's margin): there the
kernel must choose the same lag.  The kernel returns the period and the aperiodicity, not the lag; on a certified frame
  |aperiodicity - d'64(tau*)| <= 4 (tau_max + 2) u d'64(tau*)
  |period - period64| <= u' (|o| (3 + |a - 2 b| / v) + |tau* + o|),  o = (a - c) / (2 v),  u' = u / (1 - 8 u)
the second being the first-order bound of the vertex formula in fp32 on exact fp32 inputs: fl(a - c) carries u,
v = fl(fl(a - 2 b) + c) carries u (|a - 2 b| + |v|) / |v|, the division u (2 v is exact), the final sum u |tau* + o|.
Another lag fails one of the two: a lag on the path (first lag under the threshold ... end of the descent) has a d'
larger than d'(tau*) by more than the certified gap, and a lag off it has a period a sample or more away.  Frames whose
v is not safely positive (v <= 4 u (|a - 2 b| + |c|)) count as uncertified: the branch on v > 0 may go either way."""
import numpy as np

import pitch_spec as P

U = 2.0 ** -24
TIMBRES = ("harmonic", "weak_fundamental", "odd")


def tone(midi: float, timbre: str, seconds: float = 0.5, fs: int = 16000, noise: float = 0.003, seed: int = 0) -> np.ndarray:
    """A decaying harmonic tone in float64: partials h f0 <= 7.6 kHz with amplitudes 1 / h (`harmonic`), the same with
    the fundamental at 0.15 (`weak_fundamental`, -16 dB) or the odd partials only (`odd`), phases 0.7 h, envelope
    exp(-2 t), peak 0.5, plus white Gaussian noise of standard deviation `noise`."""
    f0 = 440.0 * 2.0 ** ((midi - 69.0) / 12.0)
    t = np.arange(int(round(seconds * fs))) / fs
    x = np.zeros_like(t)
    h = 1
    while h * f0 <= 7600.0:
        a = 1.0 / h
        if timbre == "weak_fundamental" and h == 1:
            a = 0.15
        if timbre == "odd" and h % 2 == 0:
            a = 0.0
        x += a * np.sin(2.0 * np.pi * h * f0 * t + 0.7 * h)
        h += 1
    x *= np.exp(-2.0 * t) * 0.5 / np.abs(x).max()
    return x + noise * np.random.default_rng(seed).standard_normal(t.size)


def compare_difference(d, e, x, w: int, hop: int, tau_max: int, exact: bool = False):
    """d [T, tau_max + 1], e [T] of one row against the spec on the same fp32 samples x [L].  exact: bit equality (an
    impulse: every entry is 0, 1 or 2, every energy 0 or 1).  Returns the largest err / bound (0 where both are 0)."""
    want_d, want_e = P.difference(np.asarray(x, dtype=np.float32).astype(np.float64), w, hop, tau_max)
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    assert d.shape == want_d.shape and e.shape == want_e.shape, (d.shape, want_d.shape, e.shape, want_e.shape)
    if exact:
        assert set(np.unique(want_d)) <= {0.0, 1.0, 2.0} and set(np.unique(want_e)) <= {0.0, 1.0}
        assert np.array_equal(d, want_d), f"d differs at (t, tau) {np.argwhere(d != want_d)[:8].tolist()}"
        assert np.array_equal(e, want_e), f"e differs at t {np.flatnonzero(e != want_e)[:8].tolist()}"
        return 0.0
    share = 0.0
    for name, got, want in (("d", d, want_d), ("e", e, want_e)):
        bound = (w + 4) * U * want
        err = np.abs(got - want)
        assert (err <= bound).all(), f"{name} beyond (W + 4) 2^-24 of the spec at {np.argwhere(err > bound)[:8].tolist()}"
        share = max(share, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    return share


def certify(d32, tau_min: int, tau_max: int, thr: float):
    """The float64 choice on d32 (the fp32 values the kernel is given) and which frames bind the kernel.
    -> dict(tau, period, aperiodicity, certified [T] bool, period_bound [T], ap_bound [T])."""
    d = np.asarray(d32, dtype=np.float32).astype(np.float64)
    tau, period, ap, margin = P.pick(d, tau_min, tau_max, float(np.float32(thr)))
    rel = 4.0 * (tau_max + 2) * U
    rows = np.arange(d.shape[0])
    a, b, c = d[rows, tau - 1], d[rows, tau], d[rows, tau + 1]
    v = a - 2.0 * b + c
    safe = v > 4.0 * U * (np.abs(a - 2.0 * b) + np.abs(c))
    o = np.where(safe, (a - c) / np.where(safe, 2.0 * v, 1.0), 0.0)
    u1 = U / (1.0 - 8.0 * U)
    period_bound = u1 * (np.abs(o) * (3.0 + np.abs(a - 2.0 * b) / np.where(safe, v, 1.0)) + np.abs(tau + o))
    return dict(tau=tau, period=period, aperiodicity=ap, certified=(margin > rel) & safe, period_bound=period_bound,
                ap_bound=rel * ap)


def compare_pick(period, aperiodicity, d32, tau_min: int, tau_max: int, thr: float, max_uncertified: float = 0.05):
    """The kernel's per-frame results against the float64 choice on the same d32.  Returns (uncertified share, largest
    period err / bound, largest aperiodicity err / bound) over the certified frames."""
    ref = certify(d32, tau_min, tau_max, thr)
    ok = ref["certified"]
    uncertified = 1.0 - ok.mean()
    assert uncertified <= max_uncertified, f"{(~ok).sum()} of {ok.size} frames uncertified: the inputs do not bind the kernel"
    period, aperiodicity = np.asarray(period, dtype=np.float64), np.asarray(aperiodicity, dtype=np.float64)
    ap_err = np.abs(aperiodicity - ref["aperiodicity"])
    bad = ok & (ap_err > ref["ap_bound"])
    assert not bad.any(), f"aperiodicity (hence the lag) differs on certified frames {np.flatnonzero(bad)[:8].tolist()}"
    p_err = np.abs(period - ref["period"])
    bad = ok & (p_err > ref["period_bound"])
    assert not bad.any(), (f"period differs on certified frames {np.flatnonzero(bad)[:8].tolist()}: got "
                           f"{period[bad][:4].tolist()}, want {ref['period'][bad][:4].tolist()} (lags {ref['tau'][bad][:4].tolist()})")
    return (float(uncertified), float((p_err[ok] / ref["period_bound"][ok]).max()),
            float((ap_err[ok] / np.maximum(ref["ap_bound"][ok], 1e-300)).max()))


def pick_frames(seed: int = 0):
    """Difference functions for the pick kernel at the default constants, fp32 [F, TAU_MAX + 1]: 0.25 s tones of the three
    timbres plus light noise, synthesised at the analysis rate (10 frames each), frames of white noise (the fallback:
    no lag under the threshold) and four frames of silence (cs = 0).  -> (d32, kinds [F] of 'tone' / 'noise' / 'silence')."""
    rows, kinds = [], []
    k = 0
    for timbre in TIMBRES:
        for midi in (21, 33.4, 45, 52.7, 60.3, 66, 72.5, 81, 90.2, 97, 103.6, 108):
            x = tone(midi, timbre, seconds=0.25, fs=P.FS_A, noise=0.003 if k % 2 else 0.02, seed=seed + k)
            d, _ = P.difference_by_correlation(x.astype(np.float32).astype(np.float64))
            rows.append(d)
            kinds += ["tone"] * d.shape[0]
            k += 1
    rng = np.random.default_rng(seed + 1000)
    d, _ = P.difference_by_correlation(0.3 * rng.standard_normal(P.W + P.TAU_MAX + 19 * P.HOP))
    rows.append(d)
    kinds += ["noise"] * d.shape[0]
    rows.append(np.zeros((4, P.TAU_MAX + 1)))
    kinds += ["silence"] * 4
    return np.concatenate(rows).astype(np.float32), np.array(kinds)
