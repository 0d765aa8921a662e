"""Specification of the time-warped band-limited read (csrc/warp_resample.hip, isi_warp_resample_f32; the resampler of
tests/resample_spec.py with a position and a cutoff per output sample), in NumPy float64; an fp32 emulation of the
kernel's weight evaluation; the cases of tests/test_warp_resample_gpu.py; the comparison both test files use; a set of
planted faults; and the float64 experiments behind GANsynth_pytorch/bend.py.  Imports nothing from the product.

    y[b, n] = sum_m  c h(c (p - m)) x[b, m]     over the integers m in [0, L) with |c (p - m)| < Z
    p = pos[b or 0, n] (float64, in source samples),  c = min(max(cut[b or 0, n], CUT_MIN), 1), CUT_MIN = fp32(0.2) (NaN: CUT_MIN)
    h(t) = sinc(t) I0(BETA sqrt(1 - (t / Z)^2)) / I0(BETA)

x is 0 outside [0, L); a position that is NaN or infinite, or whose support does not meet [0, L), gives +0.0.

The bound per output, u = 2^-24:   |got - spec| <= E_W c S1 + (N + 2) u S2
    S1  sum of |x| over the support widened by one tap on each side (a boundary tap that one arithmetic takes and the
        other does not weighs less than 2e-8 c)
    S2  sum of |w x| over the support, N its tap count: the order-free bound of an fp32 sum of N rounded products
    E_W twice the largest |w32 - w64| / c that `weights32` -- the kernel's arithmetic, operation by operation -- shows
        against the float64 weight on the grid of `measure_weight_error`.

The kernel's weight, per tap, with ip = floor(p) and frac = fp32(p - ip) taken once per output in float64:
    d = fp32(ip - m) + frac;  th = c d, tl = fma(c, d, -th) (the product's exact rest);  n = rint(th), r = (th - n) + tl
    sin(pi t) = (-1)^n r S(r^2), S the Taylor polynomial of degree 6 (|r| <= 1/2);  sinc = that / (PI32 th), 1 below 2^-20
    s = th / Z, v = s s, vl = fma(s, s, -v), u = 1 - v, ul = ((1 - u) - v) - vl (what u lost);  A(u) = sum_k a_k u^k,
    a_k = (BETA^2 / 4)^k / (k!)^2 / I0(BETA), k <= 23, by Horner in fma: the coefficients are positive and u is in [0, 1],
    nothing cancels;  window = fma(A, WIN_SLOPE ul, A): d log A / du is 7.1 at u = 1 and matters only there
    w = (c sinc) window, taken where |th| < Z."""
import math
from types import SimpleNamespace

import numpy as np

import resample_spec as R

Z, ROLLOFF, BETA = R.Z, R.ROLLOFF, R.BETA
CUT_MIN = np.float32(0.2)
U = 2.0 ** -24
# measured by measure_weight_error() on the CPU: the largest |w32 - w64| / c is 4.02 x 2^-24 (at cut 0.2, t = 0.28; the
# same arithmetic without the window's low part u_lo shows 13.3 x 2^-24: the window moves 7 times as fast as u near t = 0)
E_W = 2.0 * 4.03 * U
K_MAX = int(math.ceil(Z / float(CUT_MIN))) + 1            # taps on each side of floor(p) the kernel walks at most
OUT_POISON = 0x7FC5A5A5                                   # a NaN no kernel makes
SIN_COEF = np.array([(-1) ** k * math.pi ** (2 * k + 1) / math.factorial(2 * k + 1) for k in range(7)], dtype=np.float32)
WIN_COEF = np.array([(BETA * BETA / 4.0) ** k / math.factorial(k) ** 2 / float(R.i0(np.float64(BETA))) for k in range(24)],
                    dtype=np.float32)
WIN_SLOPE = np.float32(7.13)                              # d log A / du near u = 1, where the window is not small
MUTANTS = ("gain_without_c", "window_on_distance", "positions_float32", "fraction_sign", "edge_repeated", "cut_not_clamped")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def clamp_cut(cut):
    """the kernel's cutoff, in float64 (an fp32 cut is kept exactly): NaN and anything below CUT_MIN -> CUT_MIN, above 1 -> 1"""
    c = np.asarray(cut).astype(np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(c >= float(CUT_MIN), c, float(CUT_MIN))
    return np.minimum(c, 1.0)


def weight64(t):
    """h(t) in float64, 0 where |t| >= Z"""
    t = np.asarray(t, dtype=np.float64)
    inside = np.abs(t) < Z
    ts = np.where(inside, t, 0.0)
    h = R.sinc(ts) * R.i0(BETA * np.sqrt(1.0 - (ts / Z) ** 2)) / R.i0(np.float64(BETA))
    return np.where(inside, h, 0.0)


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64"""
    return (_f32(a).astype(np.float64) * _f32(b).astype(np.float64) + _f32(c).astype(np.float64)).astype(np.float32)


def weights32(c, frac, k):
    """(w fp32, taken bool): the kernel's arithmetic for a tap at integer distance k = floor(p) - m; c, frac fp32"""
    c, frac = _f32(c), _f32(frac)
    d = _f32(k) + frac
    th = c * d
    tl = _fma(c, d, -th)
    n = np.rint(th)
    r = (th - n) + tl
    z = r * r
    s = np.broadcast_to(SIN_COEF[6], z.shape)
    for coef in SIN_COEF[5::-1]:
        s = _fma(s, z, coef)
    sinpi = r * s
    sinpi = np.where(np.mod(n, 2.0) != 0.0, -sinpi, sinpi)
    den = np.float32(math.pi) * th
    with np.errstate(divide="ignore", invalid="ignore"):
        sinc = np.where(np.abs(th) < np.float32(2.0 ** -20), np.float32(1.0), sinpi / den).astype(np.float32)
    sc = th * np.float32(1.0 / Z)
    v = sc * sc
    vl = _fma(sc, sc, -v)
    u = np.float32(1.0) - v
    ul = ((np.float32(1.0) - u) - v) - vl
    win = np.broadcast_to(WIN_COEF[-1], u.shape)
    for coef in WIN_COEF[-2::-1]:
        win = _fma(win, u, coef)
    win = _fma(win, ul * WIN_SLOPE, win)
    w = (c * sinc) * win
    taken = np.abs(th) < np.float32(Z)
    return np.where(taken, w, np.float32(0.0)).astype(np.float32), taken


def measure_weight_error(n_frac=200, seed=0):
    """the largest |w32 - w64| / c over cuts {0.2, 0.3, 0.5, 0.7, ROLLOFF, 1} x n_frac random fractions x all taps, in
    units of 2^-24; the float64 weight takes the fp32 cut and the float64 fraction"""
    g = np.random.default_rng(seed)
    worst = 0.0
    k = np.arange(-K_MAX, K_MAX + 1, dtype=np.float64)[None, :]
    for cut in (0.2, 0.3, 0.5, 0.7, ROLLOFF, 1.0):
        c = clamp_cut(cut).astype(np.float32)
        frac = g.uniform(0.0, 1.0, n_frac)[:, None]
        w64 = float(c) * weight64(float(c) * (k + frac))
        w32, _ = weights32(c, frac.astype(np.float32), k)
        worst = max(worst, float(np.abs(w32.astype(np.float64) - w64).max()) / float(c))
    return worst / U


def warp(x, pos, cut, mutant=None, chunk=4096):
    """The specification: x [B, L], pos float64 [1 or B, N], cut [1 or B, N] -> namespace with y [B, N] float64, bound
    [B, N], zero bool [B, N] (outputs that must be +0.0).  `mutant`: one of MUTANTS, a planted fault."""
    x = np.asarray(x).astype(np.float64)                    # the kernel's cases hand in fp32 samples: kept exactly
    pos = np.asarray(pos, dtype=np.float64)
    B, L = x.shape
    N = pos.shape[1]
    c_all = clamp_cut(cut)
    if mutant == "cut_not_clamped":
        c_all = np.nan_to_num(np.asarray(cut, dtype=np.float32).astype(np.float64), nan=float(CUT_MIN))
        c_all = np.clip(c_all, 0.05, 8.0)
    if mutant == "positions_float32":
        pos = pos.astype(np.float32).astype(np.float64)
    y, bound, zero = np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N), dtype=bool)
    for b in range(B):
        for n0 in range(0, N, chunk):
            p = pos[b % pos.shape[0], n0:n0 + chunk]
            c = c_all[b % c_all.shape[0], n0:n0 + chunk]
            half = Z / c
            reach = int(min(math.ceil(half.max()), 4 * K_MAX)) + 2
            k = np.arange(-reach, reach + 1)
            with np.errstate(invalid="ignore"):
                live = np.isfinite(p) & (p > -half - 1.0) & (p < L + half)
            zero[b, n0:n0 + chunk] = ~live
            ps = np.where(live, p, 0.0)
            ip = np.floor(ps)
            frac = ps - ip
            if mutant == "fraction_sign":
                frac = -frac
            m = ip[:, None].astype(np.int64) - k[None, :]                 # distance p - m = k + frac
            dist = k[None, :] + frac[:, None]
            t = c[:, None] * dist
            inside = (m >= 0) & (m < L)
            xm = x[b][np.clip(m, 0, L - 1)]
            xs = xm if mutant == "edge_repeated" else np.where(inside, xm, 0.0)
            gain = 1.0 if mutant == "gain_without_c" else c[:, None]
            if mutant == "window_on_distance":
                ts = np.where(np.abs(t) < Z, t, 0.0)
                ds = np.clip(dist, -Z, Z)
                h = np.where(np.abs(t) < Z, R.sinc(ts) * R.i0(BETA * np.sqrt(1.0 - (ds / Z) ** 2)) / R.i0(np.float64(BETA)), 0.0)
            else:
                h = weight64(t)
            prod = gain * h * xs
            support = np.abs(t) < Z
            wide = np.abs(t) < Z + c[:, None]
            s1 = (np.abs(np.where(inside, xm, 0.0)) * wide).sum(1)
            s2 = np.abs(prod).sum(1)
            taps = (support & inside).sum(1)
            y[b, n0:n0 + chunk] = np.where(live, prod.sum(1), 0.0)
            bound[b, n0:n0 + chunk] = np.where(live, E_W * c * s1 + (taps + 2) * U * s2, 0.0)
    return SimpleNamespace(y=y, bound=bound, zero=zero)


def warp32(x, pos, cut):
    """The kernel's arithmetic in NumPy fp32: `weights32` and an fma chain over m ascending.  [B, N] float32."""
    x = np.asarray(x, dtype=np.float32)
    pos = np.asarray(pos, dtype=np.float64)
    B, L = x.shape
    N = pos.shape[1]
    c_all = clamp_cut(cut).astype(np.float32)
    out = np.zeros((B, N), dtype=np.float32)
    for b in range(B):
        p = pos[b % pos.shape[0]]
        c = c_all[b % c_all.shape[0]]
        with np.errstate(invalid="ignore"):
            live = (p >= -400.0) & (p <= L + 400.0)
        ps = np.where(live, p, 0.0)
        ip = np.floor(ps)
        frac = (ps - ip).astype(np.float32)
        reach = np.ceil(np.float32(Z) / c).astype(np.int64) + 1
        acc = np.zeros(N, dtype=np.float32)
        for k in range(K_MAX + 1, -K_MAX - 2, -1):                        # m = ip - k ascending
            m = ip.astype(np.int64) - k
            ok = live & (m >= 0) & (m < L) & (k <= reach) & (-k <= reach + 1)
            if not ok.any():
                continue
            w, _ = weights32(c, frac, np.full(N, float(k)))
            acc = np.where(ok, _fma(w, x[b][np.clip(m, 0, L - 1)], acc), acc)
        out[b] = acc
    return out


def compare(got, spec, what=""):
    """got float32 [B, N] against a `warp` result; returns the worst error / bound.  Outputs without a source are +0.0."""
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == spec.y.shape, f"{what}: shape {got.shape}"
    assert np.isfinite(got).all(), f"{what}: an output is not finite"
    assert not bits(got)[spec.zero].any(), f"{what}: an output without a source is not +0.0"
    err = np.abs(got.astype(np.float64) - spec.y)
    exact = spec.bound == 0.0
    assert not (err[exact] != 0).any(), f"{what}: an output with an empty bound is not exact"
    ratio = float((err[~exact] / spec.bound[~exact]).max()) if (~exact).any() else 0.0
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    return ratio


# ------------------------------------------------------------------------------------------------------------ the cases
KERNEL_L, KERNEL_N, KERNEL_B = (1, 2, 65, 1000), (1, 63, 64, 65, 300), (1, 3)
N_ROW_KINDS = 10


def constant_rate_rows(L, num, den):
    """positions and cuts (float64: the kernel is given them rounded to fp32) of the polyphase resampler's conversion
    num -> den (fs_in = num, fs_out = den): N = ceil(L den / num)"""
    N = -(-L * den // num)
    pos = np.arange(N, dtype=np.float64) * num / den
    return pos, np.full(N, ROLLOFF * min(1.0, den / num))


def row(kind, L, N, g):
    """one row of positions (float64) and cuts (float32): the patterns the GPU test walks"""
    n = np.arange(N, dtype=np.float64)
    rate = np.ones(N)
    if kind == 0:                                          # rate 1 on the integers
        p = n.copy()
    elif kind == 1:                                        # constant 3/2
        p, rate = 1.5 * n, np.full(N, 1.5)
    elif kind == 2:                                        # constant 2/3, from a fractional start
        p = 0.25 + n * (2.0 / 3.0)
    elif kind == 3:                                        # vibrato around rate 1
        p = n + 3.0 * np.sin(2.0 * math.pi * n / 40.0)
        rate = 1.0 + 3.0 * (2.0 * math.pi / 40.0) * np.cos(2.0 * math.pi * n / 40.0)
    elif kind == 4:                                        # a glide from rate 1 to rate 7: the cut meets its clamp
        rate = 1.0 + 6.0 * n / max(N - 1, 1)
        p = np.cumsum(rate) - rate
    elif kind == 5:                                        # decreasing: time reversal
        p = (L - 1) - 0.8 * n
    elif kind == 6:                                        # anywhere
        p = g.uniform(-5.0, L + 5.0, N)
    elif kind == 7:                                        # straddling 0 and L, out to where the support ends
        p = np.concatenate([np.linspace(-Z / ROLLOFF - 2.0, 3.0, N - N // 2), np.linspace(L - 3.0, L + Z / ROLLOFF + 2.0, N // 2)])
    elif kind == 8:                                        # far outside, infinite, NaN, between ordinary ones
        p = g.uniform(0.0, L, N)
        for i, v in enumerate((1e12, -1e12, np.inf, -np.inf, np.nan, 3e9, -3e9, 1e300)):
            p[i::11] = v
    else:                                                  # ordinary positions under the cuts 0, negative, 5 and NaN
        p = g.uniform(0.0, L, N)
    cut = (ROLLOFF * np.minimum(1.0, 1.0 / np.maximum(np.abs(rate), 1e-9))).astype(np.float32)
    if kind == 9:
        cut = np.resize(np.array([0.0, -1.0, 5.0, np.nan, 0.5], dtype=np.float32), N)
    return p, cut


def data(kind, B, L, g):
    if kind == 0:
        return g.standard_normal((B, L)).astype(np.float32)
    x = np.zeros((B, L), dtype=np.float32)
    if kind == 1:                                          # impulses at 0 and L - 1
        x[:, 0] += 1.0
        x[:, L - 1] += 1.0
        return x
    return x + np.float32(1.0)


def make_case(L, N, B, pos_batch, seed=0):
    g = np.random.default_rng([L, N, B, pos_batch, seed])
    first = (L + 3 * N + 5 * B + pos_batch + seed) % N_ROW_KINDS
    kinds = [(first + 3 * r) % N_ROW_KINDS for r in range(pos_batch)]
    rows = [row(k, L, N, g) for k in kinds]
    pos, cut = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    x = data((L + N + B + seed) % 3, B, L, g)
    return SimpleNamespace(L=L, N=N, B=B, pos_batch=pos_batch, x=x, pos=pos, cut=cut, spec=warp(x, pos, cut),
                           name=f"L={L} N={N} B={B} pos_batch={pos_batch} rows={kinds} seed={seed}")


def kernel_cases():
    """every (L, N, B, pos_batch), twice, so that every kind of row meets every size class"""
    for L in KERNEL_L:
        for N in KERNEL_N:
            for B in KERNEL_B:
                for pos_batch in sorted({1, B}):
                    for seed in (0, 1):
                        yield make_case(L, N, B, pos_batch, seed)


# ------------------------------------------------------ bending a pitch contour: the float64 arithmetic and its experiments
def curve_maps(semis, hop):
    """GANsynth_pytorch.bend.bend_maps, restated: the per-sample curve in semitones -> (r, phi, frame positions):
    r = 2^(s / 12); phi = exclusive cumsum(r), the place in the stretched sound that output sample n reads; the source
    position, in frames, of the stretched sound's frame j: phi^-1(j hop) / hop for j hop < phi(L), by linear interpolation"""
    semis = np.asarray(semis, dtype=np.float64)
    r = 2.0 ** (semis / 12.0)
    phi = np.cumsum(r) - r
    n_frames = int(math.ceil((phi[-1] + r[-1]) / hop))
    v = np.arange(n_frames, dtype=np.float64) * hop
    i = np.clip(np.searchsorted(phi, v, side="right") - 1, 0, len(r) - 1)
    return r, phi, (i + (v - phi[i]) / r[i]) / hop


def bend(x, semis, n_fft=256, hop=64, mutant=None):
    """GANsynth_pytorch.bend.bend in float64: the sound x [L] with its pitch moved by the per-sample curve `semis`, at its own
    length.  The sound is stretched by the curve's local rate (the stretch specification's STFT, phase-locked re-timing and
    inverse), then read along phi at that rate (`warp`): every instant stays where it was, every frequency is multiplied by
    r.  mutant: "no_stretch", "warp_sign", "positions_from_phi" -- planted faults of the path."""
    import stft_stretch_spec as V
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    r, phi, frames = curve_maps(semis, hop)
    T, extra = -(-L // hop), n_fft // hop - 1
    cut = ROLLOFF * np.minimum(1.0, 1.0 / r)
    tail = int(math.ceil((Z / cut.min() + 2.0) / hop))
    T_all = T + extra + tail
    if mutant == "positions_from_phi":
        frames = (phi[np.minimum(np.arange(len(frames)) * hop, L - 1)]) / hop
    if mutant == "no_stretch":
        frames = np.arange(len(frames), dtype=np.float64)
    pos = np.concatenate([np.minimum(frames, T_all - 1), np.arange(T, T_all, dtype=np.float64)]).astype(np.float32)[None]
    X = V.stft(x, n_fft, hop, T_all)
    Y = V.stretch(V.pack(X), pos, hop).out[0]
    z = V.istft(Y, n_fft, hop, (len(frames) + tail) * hop)
    if mutant == "warp_sign":
        r = 1.0 / r
        phi = np.cumsum(r) - r
    return warp(z[None], phi[None], cut[None]).y[0]


FS, F0, N_EXP = 16000, 440.0, 16000
TRIM = 1500


def vibrato_curve(L, depth_cents=50.0, rate_hz=6.0, fs=FS):
    return depth_cents / 100.0 * np.sin(2.0 * math.pi * rate_hz * np.arange(L) / fs)


def glide_curve(L, semitones=3.0):
    return semitones * np.arange(L) / L


def tone_along(semis, f0=F0, fs=FS, attack_s=0.010):
    """partials 1, 0.5, 0.25 of f0 2^(semis / 12) (the phase is the running sum of the frequency), a 10 ms attack"""
    semis = np.asarray(semis, dtype=np.float64)
    f = f0 * 2.0 ** (semis / 12.0)
    phase = 2.0 * math.pi * (np.cumsum(f) - f) / fs
    attack = np.minimum(np.arange(len(semis)) / (attack_s * fs), 1.0)
    return attack * sum(a * np.sin(k * phase) for k, a in ((1, 1.0), (2, 0.5), (3, 0.25)))


def track_cents(y, semis_ideal, f0=F0, fs=FS, smooth=64, trim=TRIM):
    """the pitch of y against f0 2^(semis_ideal / 12), in cents per sample: the instantaneous frequency of the band-passed
    fundamental (0.7 f0 .. 1.45 f0, an analytic signal by the FFT), smoothed over `smooth` samples, `trim` samples dropped
    at each end.  (rms, max |.|)"""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    spec = np.fft.fft(y)
    freq = np.fft.fftfreq(n, 1.0 / fs)
    spec[(freq < 0.7 * f0) | (freq > 1.45 * f0)] = 0.0
    phase = np.unwrap(np.angle(np.fft.ifft(2.0 * spec)))
    inst = np.diff(phase) * fs / (2.0 * math.pi)
    inst = np.convolve(inst, np.ones(smooth) / smooth, mode="same")
    semis_ideal = np.broadcast_to(np.asarray(semis_ideal, dtype=np.float64), (n,))
    ideal = f0 * 2.0 ** (0.5 * (semis_ideal[1:] + semis_ideal[:-1]) / 12.0)
    ideal = np.convolve(ideal, np.ones(smooth) / smooth, mode="same")
    cents = 1200.0 * np.log2(inst[trim:-trim] / ideal[trim:-trim])
    return float(np.sqrt(np.mean(cents ** 2))), float(np.abs(cents).max())


def level_ratio(y, x, trim=TRIM):
    return float(np.sqrt(np.mean(y[trim:-trim] ** 2) / np.mean(x[trim:-trim] ** 2)))


def experiment_flatten(mutant=None, sharp_cents=0.0, bend_fn=None):
    """a +-50 cent, 6 Hz vibrato (on a tone `sharp_cents` sharp) flattened with its known curve.  Returns a namespace: left
    (rms, max) in cents against the flat 440 Hz, source (the same of the untreated sound), level, length.  bend_fn(x, semis)
    replaces the float64 path (the GPU test hands the product in)."""
    own = sharp_cents / 100.0 + vibrato_curve(N_EXP)
    x = tone_along(own)
    y = (bend_fn or (lambda a, s: bend(a, s, mutant=mutant)))(x, -own)
    return SimpleNamespace(left=track_cents(y, 0.0), source=track_cents(x, 0.0), level=level_ratio(y, x), length=len(y))


def experiment_vibrato(mutant=None, bend_fn=None):
    """the same vibrato added to a flat tone, against the ideal vibrato tone's pitch"""
    x = tone_along(np.zeros(N_EXP))
    want = vibrato_curve(N_EXP)
    y = (bend_fn or (lambda a, s: bend(a, s, mutant=mutant)))(x, want)
    return SimpleNamespace(left=track_cents(y, want), source=track_cents(x, want), level=level_ratio(y, x), length=len(y))


def experiment_glide(mutant=None, bend_fn=None):
    """a linear glide of +3 semitones over the sound, against the ideal"""
    x = tone_along(np.zeros(N_EXP))
    want = glide_curve(N_EXP)
    y = (bend_fn or (lambda a, s: bend(a, s, mutant=mutant)))(x, want)
    return SimpleNamespace(left=track_cents(y, want), source=track_cents(x, want), level=level_ratio(y, x), length=len(y))


def contour(audio, fs_hz=FS, periods=4.0, w=None):
    """GANsynth_pytorch.pitch.pitch_contour in float64 (tests/pitch_spec.py's YIN): the clip's pitch gives the period, the
    window is about `periods` of them (W = 64 ceil(periods period / 64) in [256, 3072]; `w` overrides), hop W / 4, lags
    limited to floor(0.7 period) .. ceil(1.45 period) + 2.  (midi [T], voiced [T], times_s [T], clip pitch)"""
    import pitch_spec as P
    clip_midi, _ = P.estimate(audio, fs_hz)
    period = P.FS_A / (440.0 * 2.0 ** ((clip_midi - 69.0) / 12.0))
    W = w or min(max(64 * int(math.ceil(periods * period / 64.0)), 256), 3072)
    hop, tau_min, tau_max = W // 4, int(math.floor(0.7 * period)), int(math.ceil(1.45 * period)) + 2
    x = P.analysis_signal(audio, fs_hz, W, tau_max)
    d, e = P.difference_by_correlation(x, W, hop, tau_max)
    _, per, ap, _ = P.pick(d, tau_min, tau_max)
    _, _, midi, voiced = P.clip(per, ap, e)
    times = (np.arange(len(midi)) * hop + (W + period) / 2.0) / P.FS_A
    return midi, voiced, times, clip_midi


def contour_curve(midi, voiced, times, clip_midi, L, fs_hz=FS, max_correction=1.5):
    """the contour per output sample: frames that are unvoiced or further than `max_correction` semitones from the clip's
    pitch take the nearest accepted frame's value; linear between frame times, held outside"""
    ok = voiced & (np.abs(midi - clip_midi) <= max_correction)
    idx = np.flatnonzero(ok)
    nearest = idx[np.abs(np.arange(len(midi))[:, None] - idx[None, :]).argmin(1)]
    return np.interp(np.arange(L) / fs_hz, times, midi[nearest])


def experiment_flatten_tracked(w=None, bend_fn=None, contour_fn=None):
    """a tone 30 cents sharp with the vibrato, flattened to MIDI 69 by its own tracked contour.  contour_error: the contour
    against the sound's true curve, in cents (rms, max) over the same trimmed span."""
    own = 0.30 + vibrato_curve(N_EXP)
    x = tone_along(own)
    midi, voiced, times, clip_midi = (contour_fn or (lambda a: contour(a, w=w)))(x)
    seen = contour_curve(midi, voiced, times, clip_midi, N_EXP)
    y = (bend_fn or bend)(x, 69.0 - seen)
    off = 100.0 * (seen - 69.0 - own)[TRIM:-TRIM]
    return SimpleNamespace(left=track_cents(y, 0.0), source=track_cents(x, 0.0), level=level_ratio(y, x), length=len(y),
                           contour_error=(float(np.sqrt(np.mean(off ** 2))), float(np.abs(off).max())), W=w)
