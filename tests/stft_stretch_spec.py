"""Float64 specification (numpy) of isi_stft_stretch_f32 (csrc/stft_stretch.hip): an STFT re-timed along a list of source
positions with identity phase locking; its float32 model in the kernel's order, with planted faults; the cases of
tests/test_stft_stretch_gpu.py with their data; the comparison both test files use; and the float64 experiment behind the
choice of the method.  No GPU, none of the project's kernels.

Layouts (include/isi_hip.h): X [B, T, 2F] real block | imaginary block, DC dropped (bin j is DFT bin j + 1 of n_fft = 2F);
pos [pos_batch, T_out] source positions in frames; out [B, T_out, 2F].

Source, per (b, t, j): P = fl(fl(re re) + fl(im im)) in float32 (decided there, so that the peaks are exact properties of the
data), A = sqrt P, phi = atan2(im, re), Omega_j = 2 pi ((j + 1) hop mod n_fft) / n_fft, Omegafull_j = 2 pi (j + 1) hop / n_fft,
dev[t] = wrap(phi[t+1] - phi[t] - Omega_j), wrap = principal value in (-pi, pi].
    peak:  P > 0 and for d = 1, 2: P[j] > P[j-d] and P[j] >= P[j+d] (neighbours outside [0, F) do not object)
    near[t, j] = the peak nearest to j, the lower one on a tie; j itself in a frame without a peak
Output frame u: p = pos[u] clamped to [0, T-1] (NaN: 0), t = min(floor p, T-2), f = p - t, ta = t if f < 0.5 else t + 1,
    M = (1 - f) A[t] + f A[t+1],  D = Omega + ((1 - f) dev[max(t-1, 0)] + f dev[t])
    u == 0:  Phi = phi[t] + f (Omegafull + dev[t])
    u > 0:   n = near[ta];  Phi[j] = wrap((Phi'[n] + D[n]) + (phi[ta, j] - phi[ta, n]))
    out = M (cos Phi | sin Phi)
The leading copy run: c = the largest count with pos[0] an integer in [0, T-1] and pos[u] == pos[0] + u <= T-1 for u < c;
those frames are the source's floats bit for bit and Phi of frame c - 1 is that frame's phi.

The bound, element by element as complex numbers, u = 2^-24: |got - spec| <= M E_phase + E_mag.
    E_at = 2^-21: atan2f within 2 ulp of an angle of at most pi.
    E_om = 3u Omega: the quotient, the product and float32(2 pi); E_omfull = 4u Omegafull (the integer's conversion too).
    E_dev = 2 E_at + u |phi1 - phi0| + E_om + u |d| + 4u (|d| + 2 pi), d = phi1 - phi0 - Omega: two angles, two subtractions,
            and the wrap (quotient, ceiling times float32(2 pi), last subtraction).  The wrap is a step: the data keep every d
            at least WRAP_MARGIN from an odd multiple of pi (`make_source` turns bins where it is not).
    E_D   = E_om + (1-f) E_dev[tm] + f E_dev[t] + u (|d0| + |(1-f) d0| + |f d1| + |(1-f) d0 + f d1| + |D|): 1 - f, two
            products, two sums.
    E_Phi, copied frame: E_at.  Frame 0: E_at + f (E_omfull + E_dev[t]) + u f |s| + u |f s| + u |Phi|, s = Omegafull + dev[t].
    E_Phi, u > 0: E_Phi'[n] + E_D[n] + u a + (n != j) (2 E_at + u |r|) + u (a + |r|) + 4u (a + |r| + 2 pi),
            a = max(|Phi'[n]|, pi) + |D[n]|, r = phi[ta, j] - phi[ta, n]: the chain's error is carried from frame to frame along
            the `near` path; Phi's own wrap needs no margin (2 pi more or less is the same element).
    E_phase = E_Phi + 1.5 x 2^-22 + 2u: sine and cosine within 2 ulp of a value below 1, the two products.
    E_mag = 3u M + u A[t]: the correctly rounded roots, 1 - f, two products and a sum.
Copied frames are compared bit for bit, `near` (which the kernel leaves in its workspace) exactly, and an element with
M == 0 must be 0."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

PI = math.pi
U = 2.0 ** -24
E_AT = 2.0 ** -21
WRAP_MARGIN = 1e-3
OUT_POISON = 0x7FC5A5A5          # a NaN no kernel makes
NO_PEAK = 2 ** 30
MUTANTS = ("no_lock", "lock_without_relative_phase", "advance_from_t_not_t_minus_1", "omega_not_reduced", "no_dev_wrap",
           "nearest_frame_always_floor", "tie_to_upper_peak", "copy_recomputed", "magnitude_from_ta_only")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def wrap(d):
    """principal value in (-pi, pi]"""
    d = np.asarray(d)
    two_pi, pi = d.dtype.type(2.0 * PI), d.dtype.type(PI)
    return d - two_pi * np.ceil((d - pi) / two_pi)


def omegas(F, hop, dtype=np.float64, reduced=True):
    """Omega (reduced in integers) or Omegafull, [F]"""
    n_fft = 2 * F
    m = np.arange(1, F + 1, dtype=np.int64) * hop
    if reduced:
        m = m % n_fft
    return dtype(2.0 * PI) * (m.astype(dtype) / dtype(n_fft))


def power(X):
    """P [B, T, F] float32: two rounded products and a rounded sum, as the kernel forms it"""
    X = np.asarray(X, dtype=np.float32)
    F = X.shape[-1] // 2
    re, im = X[..., :F], X[..., F:]
    return (re * re).astype(np.float32) + (im * im).astype(np.float32)


def peaks_and_near(P, tie_to_upper=False):
    """P float32 [..., F] -> (peak bool, near int64, tie bool: bins with two nearest peaks)"""
    F = P.shape[-1]
    peak = P > 0
    for d in (1, 2):
        if d < F:
            peak[..., d:] &= P[..., d:] > P[..., :-d]
            peak[..., :-d] &= P[..., :-d] >= P[..., d:]
    j = np.broadcast_to(np.arange(F, dtype=np.int64), P.shape)
    lo = np.maximum.accumulate(np.where(peak, j, -1), axis=-1)
    hi = np.minimum.accumulate(np.where(peak, j, NO_PEAK)[..., ::-1], axis=-1)[..., ::-1]
    both = (lo >= 0) & (hi < NO_PEAK)
    lower = (j - lo < hi - j) if tie_to_upper else (j - lo <= hi - j)
    near = np.where(both, np.where(lower, lo, hi), np.where(lo >= 0, lo, np.where(hi < NO_PEAK, hi, j)))
    return peak, near, both & (j - lo == hi - j) & (lo != hi)


def prepare(X, hop, dtype=np.float64, mutant=None):
    """what the preparation pass leaves per source frame, and (float64) the bound's parts"""
    X32 = np.asarray(X, dtype=np.float32)
    B, T, F2 = X32.shape
    F = F2 // 2
    P = power(X32)
    A = np.sqrt(P.astype(dtype))
    phi = np.arctan2(X32[..., F:].astype(dtype), X32[..., :F].astype(dtype))
    om, omfull = omegas(F, hop, dtype), omegas(F, hop, dtype, reduced=False)
    if mutant == "omega_not_reduced":
        om = omfull
    d = (phi[:, 1:] - phi[:, :-1]) - om
    dev = d if mutant == "no_dev_wrap" else wrap(d)
    peak, near, tie = peaks_and_near(P, tie_to_upper=mutant == "tie_to_upper_peak")
    s = SimpleNamespace(B=B, T=T, F=F, A=A, phi=phi, dev=dev, om=om, omfull=omfull, peak=peak, near=near, tie=tie, d=d)
    if dtype == np.float64:
        s.e_om = 3 * U * om
        s.e_dev = 2 * E_AT + U * np.abs(phi[:, 1:] - phi[:, :-1]) + s.e_om + U * np.abs(d) + 4 * U * (np.abs(d) + 2 * PI)
        s.margin = PI - np.abs(wrap(d))
    return s


def where(p, T):
    """(t, f, ta, tm) of one position (a float32)"""
    p = float(p)
    if not p >= 0.0:
        p = 0.0
    p = min(p, float(T - 1))
    t = min(int(math.floor(p)), T - 2)
    f = p - t
    return t, f, (t if f < 0.5 else t + 1), max(t - 1, 0)


def copy_run(row, T):
    """the leading copy run of one row of positions"""
    p0 = float(row[0])
    if not (0.0 <= p0 <= T - 1 and p0 == math.floor(p0)):
        return 0
    c = 0
    while c < len(row) and float(row[c]) == p0 + c and float(row[c]) <= T - 1:
        c += 1
    return c


def stretch(X, pos, hop, dtype=np.float64, mutant=None, src=None, copy=True):
    """The specification (dtype float64) or its float32 model in the kernel's order (dtype float32; `mutant`: one of MUTANTS).
    Returns a namespace: out complex [B, T_out, F] (float64) or float [B, T_out, 2F] (float32); for float64 also bound
    [B, T_out, F], copied bool [B, T_out], M and Phi.  copy=False: without the copy-run rule (the formula on every frame)."""
    X32 = np.asarray(X, dtype=np.float32)
    pos = np.asarray(pos, dtype=np.float32)
    s = src if src is not None else prepare(X32, hop, dtype, mutant)
    B, T, F = s.B, s.T, s.F
    T_out = pos.shape[1]
    f64 = dtype == np.float64
    j = np.arange(F)
    M_all, Phi_all = np.zeros((B, T_out, F), dtype), np.zeros((B, T_out, F), dtype)
    E_all, A0_all = np.zeros((B, T_out, F)), np.zeros((B, T_out, F))
    copied = np.zeros((B, T_out), dtype=bool)
    raw = np.zeros((B, T_out, 2 * F), dtype=np.float32)
    for b in range(B):
        row = pos[b % pos.shape[0]]
        c = copy_run(row, T) if copy else 0
        Phi = E = None
        for u in range(T_out):
            if u < c:
                t = int(row[0]) + u
                copied[b, u] = True
                raw[b, u] = X32[b, t]
                Phi, E = s.phi[b, t], np.full(F, E_AT)
                M_all[b, u], Phi_all[b, u] = s.A[b, t], Phi
                continue
            t, f, ta, tm = where(row[u], T)
            if mutant == "nearest_frame_always_floor":
                ta = t
            if mutant == "advance_from_t_not_t_minus_1":
                tm = t
            f = dtype(f)
            g = dtype(1.0) - f
            A0, A1, d0, d1 = s.A[b, t], s.A[b, t + 1], s.dev[b, tm], s.dev[b, t]
            M = s.A[b, ta] if mutant == "magnitude_from_ta_only" else g * A0 + f * A1
            mix = g * d0 + f * d1
            D = s.om + mix
            if f64:
                e_D = s.e_om + g * s.e_dev[b, tm] + f * s.e_dev[b, t] + U * (np.abs(d0) + np.abs(g * d0) + np.abs(f * d1)
                                                                             + np.abs(mix) + np.abs(D))
            if u == 0:
                s0 = s.omfull + d1
                Phi_new = s.phi[b, t] + f * s0
                if f64:
                    E = E_AT + f * (4 * U * s.omfull + s.e_dev[b, t]) + U * f * np.abs(s0) + U * np.abs(f * s0) + U * np.abs(Phi_new)
            else:
                n = j if mutant == "no_lock" else s.near[b, ta]
                ph = s.phi[b, ta]
                r = ph - ph[n]
                if mutant == "lock_without_relative_phase":
                    r = np.zeros_like(r)
                Phi_new = wrap((Phi[n] + D[n]) + r)
                if f64:
                    a = np.maximum(np.abs(Phi[n]), PI) + np.abs(D[n])
                    E = (E[n] + e_D[n] + U * a + np.where(n == j, 0.0, 2 * E_AT + U * np.abs(r)) + U * (a + np.abs(r))
                         + 4 * U * (a + np.abs(r) + 2 * PI))
            Phi = Phi_new
            M_all[b, u], Phi_all[b, u] = M, Phi
            if f64:
                E_all[b, u], A0_all[b, u] = E, A0
    if not f64:
        out = np.concatenate([M_all * np.cos(Phi_all), M_all * np.sin(Phi_all)], -1).astype(np.float32)
        if mutant != "copy_recomputed":
            out[copied] = raw[copied]
        return SimpleNamespace(out=out)
    out = M_all * np.exp(1j * Phi_all)
    Xc = X32[..., :F].astype(np.float64) + 1j * X32[..., F:].astype(np.float64)
    for b in range(B):
        row = pos[b % pos.shape[0]]
        for u in np.nonzero(copied[b])[0]:
            out[b, u] = Xc[b, int(row[0]) + u]
    bound = np.abs(M_all) * (E_all + 1.5 * 2.0 ** -22 + 2 * U) + 3 * U * np.abs(M_all) + U * A0_all
    bound[copied] = 0.0
    return SimpleNamespace(out=out, bound=bound, copied=copied, raw=raw, M=M_all, Phi=Phi_all, src=s)


# ------------------------------------------------------------------------------------------------------------ the cases
KERNEL_F, KERNEL_T, KERNEL_B = (1, 2, 5, 64, 130, 1024), (2, 3, 17, 40), (1, 3)
N_POSITION_KINDS = 8


def case_hop(F):
    """a hop that divides n_fft = 2F: n_fft / 4 where that is an integer, else the largest divisor of 2F at or below F / 2"""
    return next((h for h in range(max(F // 2, 1), 0, -1) if (2 * F) % h == 0), 1)


def t_outs(T):
    return sorted({1, 2, T, 2 * T + 1})


def make_source(B, T, F, seed=0):
    """X float32 [B, T, 2F] and its float64 preparation.  Frames cycle, by (t + b) % 6, through: random bins (lognormal
    moduli); a silent frame; random; equal magnitudes in every bin (the 8 symmetries of one (a, b): P ties bit for bit);
    a loud peak that moves one bin per frame; loud peaks at bins 0 and F - 1 and a plateau of three equal loud bins.  Every
    argument of dev's wrap is then moved at least WRAP_MARGIN from an odd multiple of pi by turning a random bin."""
    g = np.random.default_rng([B, T, F, seed])
    hop = case_hop(F)
    Z = np.exp(g.standard_normal((B, T, F))) * np.exp(1j * g.uniform(-PI, PI, (B, T, F)))
    fixed = np.zeros((B, T, F), dtype=bool)               # bins the margin repair must not turn
    X = np.concatenate([Z.real, Z.imag], -1).astype(np.float32)
    for b in range(B):
        for t in range(T):
            kind = (t + b) % 6
            if kind == 1:
                X[b, t] = 0.0
                fixed[b, t] = True
            elif kind == 3:
                a, c = np.float32(g.uniform(0.3, 2.0)), np.float32(g.uniform(0.3, 2.0))
                sym = g.integers(0, 8, F)
                re, im = np.where(sym & 1, c, a), np.where(sym & 1, a, c)
                X[b, t, :F] = np.where(sym & 2, -re, re)
                X[b, t, F:] = np.where(sym & 4, -im, im)
                fixed[b, t] = True
            elif kind == 4:
                X[b, t, [(t * 1 + 3 * b) % F, F + (t + 3 * b) % F]] *= np.float32(40.0)
            elif kind == 5:
                X[b, t, [0, F - 1, F, 2 * F - 1]] *= np.float32(30.0)
                if F >= 12:
                    a, c = np.float32(25.0), np.float32(31.0)
                    k = F // 2
                    X[b, t, k:k + 3], X[b, t, F + k:F + k + 3] = [a, c, -a], [c, -a, c]
                    fixed[b, t, k:k + 3] = True
    for _ in range(200):
        s = prepare(X, hop)
        bad = np.argwhere(s.margin < WRAP_MARGIN)
        if not len(bad):
            break
        for b, t, k in bad:
            tt = t + 1 if not fixed[b, t + 1, k] else t
            assert not fixed[b, tt, k], "two frames that cannot be turned are neighbours"
            z = complex(X[b, tt, k], X[b, tt, F + k]) * np.exp(1j * g.uniform(0.1, 1.0))
            X[b, tt, k], X[b, tt, F + k] = z.real, z.imag
    else:
        raise AssertionError("wrap ties remain")
    return SimpleNamespace(B=B, T=T, F=F, hop=hop, X=X, src=s)


def position_row(kind, T, T_out, g):
    """one row of positions (float64 before the single rounding): the patterns the issue lists"""
    u = np.arange(T_out, dtype=np.float64)
    if kind == 0:                                          # a uniform stretch from frame 0: a copy run of 1
        return u * ((T - 1) / max(T_out - 1, 1))
    if kind == 1:                                          # rate 1 as long as the source lasts (a copy run of min(T, T_out)), then frozen
        return np.minimum(u, T - 1)
    if kind == 2:                                          # no copy run: a fractional start
        return np.minimum(0.25 + 0.7 * u, T - 1)
    if kind == 3:                                          # a frozen frame
        return np.full(T_out, min(1.5, T - 1.0))
    if kind == 4:                                          # decreasing
        return (T - 1) - u * ((T - 1) / max(T_out - 1, 1)) * 0.9
    if kind == 5:                                          # outside the source, NaN, infinities
        p = g.uniform(-3.0, T + 2.0, T_out)
        p[::5] = np.nan
        p[1::7] = np.inf
        p[3::7] = -np.inf
        p[2::9] = -0.5
        p[4::9] = T - 0.5
        return p
    if kind == 6:                                          # anywhere
        return g.uniform(0.0, T - 1.0, T_out)
    p = np.minimum(1.0 + u, T - 1)                         # a copy run from frame 1 of up to three frames, then half rate
    p[3:] = np.minimum(p[2] + 0.5 * (u[3:] - 2.0), T - 1) if T_out > 3 else p[3:]
    return p


def make_case(source, T_out, pos_batch, seed=0):
    g = np.random.default_rng([source.B, source.T, source.F, T_out, pos_batch, seed])
    first = (T_out + 3 * pos_batch + source.T + source.F + seed) % N_POSITION_KINDS
    pos = np.stack([position_row((first + 3 * r) % N_POSITION_KINDS, source.T, T_out, g) for r in range(pos_batch)])
    pos = pos.astype(np.float32)
    spec = stretch(source.X, pos, source.hop, src=source.src)
    return SimpleNamespace(B=source.B, T=source.T, F=source.F, hop=source.hop, T_out=T_out, pos_batch=pos_batch, X=source.X, pos=pos,
                           spec=spec, name=f"B={source.B} T={source.T} F={source.F} T_out={T_out} pos_batch={pos_batch} hop={source.hop}")


def kernel_cases(T, F):
    for B in KERNEL_B:
        source = make_source(B, T, F)
        for pos_batch in sorted({1, B}):
            for T_out in t_outs(T):
                yield make_case(source, T_out, pos_batch)


def compare(got, case, what=None):
    """got float32 [B, T_out, 2F] against the case's specification; returns the worst error / bound.  Copied frames bit for bit."""
    what = what or case.name
    s, F = case.spec, case.F
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == (case.B, case.T_out, 2 * F), f"{what}: shape {got.shape}"
    assert np.array_equal(bits(got)[s.copied], bits(s.raw)[s.copied]), f"{what}: a frame of the copy run is not the source's bits"
    z = got[..., :F].astype(np.float64) + 1j * got[..., F:].astype(np.float64)
    assert np.isfinite(z).all(), f"{what}: an element is not finite"
    live = ~s.copied[..., None] & np.ones_like(s.bound, dtype=bool)
    err = np.abs(z - s.out)
    zero = live & (s.M == 0)
    assert not (err[zero] != 0).any(), f"{what}: an element without magnitude is not 0"
    live &= s.M != 0
    ratio = float((err[live] / s.bound[live]).max()) if live.any() else 0.0
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    return ratio


# -------------------------------------------------------------------------- the helper's STFT pair in float64, the experiment
def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * PI * np.arange(n_fft) / n_fft)


def stft(x, n_fft, hop, n_frames):
    """x [L] -> complex [n_frames, n_fft / 2]: frame t starts n_fft - hop samples before sample t hop; DC dropped"""
    left = n_fft - hop
    total = (n_frames - 1) * hop + n_fft
    xp = np.zeros(total)
    n = min(len(x), total - left)
    xp[left:left + n] = x[:n]
    frames = np.stack([xp[t * hop:t * hop + n_fft] for t in range(n_frames)]) * hann(n_fft)
    return np.fft.rfft(frames, axis=-1)[:, 1:]


def istft(X, n_fft, hop, L):
    """the helper's synthesis: inverse real DFT without DC, window w / (overlap sums of w^2), overlap-add from n_fft - hop"""
    w = hann(n_fft)
    den = np.zeros(n_fft)
    for jj in range(-(n_fft // hop), n_fft // hop + 1):
        lo, hi = max(0, -jj * hop), min(n_fft, n_fft - jj * hop)
        if lo < hi:
            den[lo:hi] += w[lo + jj * hop:hi + jj * hop] ** 2
    full = np.concatenate([np.zeros((X.shape[0], 1)), X], -1)
    frames = np.fft.irfft(full, n=n_fft, axis=-1) * (w / den)
    left, out = n_fft - hop, np.zeros(X.shape[0] * hop + n_fft)
    for t in range(X.shape[0]):
        out[t * hop:t * hop + n_fft] += frames[t]
    return out[left:left + L]


def pack(X):
    """complex [T, F] -> the kernel's [1, T, 2F]"""
    return np.concatenate([X.real, X.imag], -1)[None].astype(np.float32)


def positions(n_frames, factor=None, n_out=None, keep_head=0, keep_tail=0):
    """GANsynth_pytorch.stretch.stretch_positions, restated: float64, rounded once"""
    if n_out is None:
        n_out = max(1, int(round(n_frames * factor)))
    mid_out, mid_in = n_out - keep_head - keep_tail, n_frames - keep_head - keep_tail
    p = np.concatenate([np.arange(keep_head, dtype=np.float64),
                        keep_head + np.arange(mid_out, dtype=np.float64) * (mid_in / mid_out),
                        n_frames - keep_tail + np.arange(keep_tail, dtype=np.float64)])
    return p.astype(np.float32)


def tone(L, f0, fs=16000.0, scale=1.0, attack_s=0.010):
    """three decaying partials of f0 with a 10 ms attack; `scale` stretches the envelope's time axis (the ideally stretched
    sound keeps its frequencies)"""
    n = np.arange(L) / fs
    env_t = n / scale
    attack = np.minimum(env_t / attack_s, 1.0)
    x = sum(amp * np.exp(-env_t * decay) * np.sin(2 * PI * f0 * k * n) for k, amp, decay in ((1, 1.0, 6.0), (2, 0.5, 9.0), (3, 0.25, 14.0)))
    return attack * x


def spectral_convergence(y, ideal, n_fft, hop):
    T = len(ideal) // hop
    a, b = np.abs(stft(y, n_fft, hop, T)), np.abs(stft(ideal, n_fft, hop, T))
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def stretch_audio(x, factor, n_fft, hop, mutant=None):
    """time_stretch in numpy: the STFT of the zero-padded sound, the stretched positions followed by the trailing frames
    at rate 1, the specification (or a mutant of the float64 arithmetic), the inverse"""
    T, extra = len(x) // hop, n_fft // hop - 1
    X = stft(x, n_fft, hop, T + extra)
    T_out = max(1, int(round(T * factor)))
    pos = np.concatenate([positions(T, n_out=T_out), np.arange(T, T + extra, dtype=np.float32)])[None]
    Y = stretch(pack(X), pos, hop, mutant=mutant).out[0]
    return istft(Y, n_fft, hop, T_out * hop)


def resample_bandlimited(y, num, den, L, zeros=24):
    """y at rate num read at rate den (a float64 windowed-sinc interpolation): sample i of the result is y(i num / den)"""
    ratio = num / den
    cutoff = min(1.0, 1.0 / ratio)
    out = np.zeros(L)
    half = int(math.ceil(zeros / cutoff))
    for i in range(L):
        c = i * ratio
        k = np.arange(max(0, int(c) - half), min(len(y), int(c) + half + 1))
        if not len(k):
            continue
        d = (k - c) * cutoff
        win = np.where(np.abs(d) < zeros, 0.5 + 0.5 * np.cos(PI * d / zeros), 0.0)
        out[i] = cutoff * np.sum(y[k] * np.sinc(d) * win)
    return out


def experiment_stretch(factor, T=64, n_fft=256, hop=64, f0=440.0):
    """(locked, plain vocoder, rms of locked / rms of ideal, of plain / ideal): spectral convergence against the ideal"""
    x = tone(T * hop, f0)
    T_out = max(1, int(round(T * factor)))
    ideal = tone(T_out * hop, f0, scale=T_out / T)
    locked = stretch_audio(x, factor, n_fft, hop)
    plain = stretch_audio(x, factor, n_fft, hop, mutant="no_lock")
    rms = lambda v: float(np.sqrt(np.mean(v ** 2)))                                          # noqa: E731
    return (spectral_convergence(locked, ideal, n_fft, hop), spectral_convergence(plain, ideal, n_fft, hop),
            rms(locked) / rms(ideal), rms(plain) / rms(ideal))


def semitone_ratio(semitones, max_denominator=512):
    r = Fraction(2.0 ** (semitones / 12.0)).limit_denominator(max_denominator)
    return r.numerator, r.denominator


def experiment_transpose(semitones, num, den, T=64, n_fft=256, hop=64, f0=440.0):
    """(transposed, untransposed): spectral convergence against the partials synthesised at (num / den) f0"""
    L = T * hop
    x = tone(L, f0)
    y = stretch_audio(x, num / den, n_fft, hop)
    z = resample_bandlimited(y, num, den, L)
    ideal = tone(L, f0 * num / den)
    return spectral_convergence(z, ideal, n_fft, hop), spectral_convergence(x, ideal, n_fft, hop)
