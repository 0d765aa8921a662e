"""Float64 specification (numpy) of the two kernels of csrc/spec_splice.hip -- isi_spec_splice_f32, the phase-locked splice of
regenerated STFT frames into an original's STFT, and isi_spec_splice_blend_f32, the sample blend behind it --, the cases of
tests/test_spec_splice_gpu.py with their data, and the comparison both test files use.  No GPU, none of the project's kernels.

Layouts (include/isi_hip.h): stft [B, T, 2F] real block | imaginary block; a, ph [B, T, F]; w [w_batch, T, F]; audio [B, L];
touched [B, T_frames] bytes.

The splice, per (b, k) row: a run is a maximal range [t0, t1) of frames with w > 0; phi_o / Ao = angle / modulus of the
original's bin, psi = ph, As = the magnitude isi_spec_to_stft_f32 forms from `a`; wrap = principal value in (-pi, pi].
    w == 0            the original's two floats, bit for bit
    both neighbours   c = wrap(phi_o[t1] - phi_o[t0-1] - (psi[t1] - psi[t0-1])) / (t1 - t0 + 1)
                      phi[t] = phi_o[t0-1] + (psi[t] - psi[t0-1]) + (t - t0 + 1) c
    t0 == 0 only      phi[t] = phi_o[t1] - (psi[t1] - psi[t])
    t1 == T only      phi[t] = phi_o[t0-1] + (psi[t] - psi[t0-1])
    whole row         phi[t] = psi[t]; with w == 1 the bits isi_spec_to_stft_f32 writes
    magnitude         As where w == 1, else exp((1 - w) log Ao + w log As); exactly 0 when Ao == 0 or As <= 0: the geometric
                      mean with a silent side is silence (log 0 = -inf), and a non-positive `a` has no logarithm
    out = magnitude (cos phi | sin phi)

The bound (DESIGN.md, section "Phase-locked splice"), derived from that arithmetic in float32, u = 2^-24, element by element
as complex numbers: |got - spec| <= Amag E_phase + E_mag.
    E_at = 2^-21: atan2f within 2 ulp of an angle of at most pi (ulp 2^-22).
    E_phase = E_phi + 1.5 x 2^-22 + 2u: sine and cosine within 2 ulp of a value below 1 (2^-22 each, sqrt 2 together),
              two roundings of the products.
    E_phi, both neighbours: E_at + u |psi - psi_a| + u |phi_a + (psi - psi_a)| + j E_c + u |j c| + u |phi|, j = t - t0 + 1,
              E_c = E_d / (n + 1) + u |c|,
              E_d = 2 E_at + u |phi_b - phi_a| + u |psi_b - psi_a| + u |d| + 4u (|d| + 2 pi): the two angles, the three
              subtractions, and the wrap (d - pi, the quotient and its ceiling's product with float32(2 pi), whose own
              error is below u 2 pi per turn, and the last subtraction).  The wrap is a step: the data keep every d at
              least WRAP_MARGIN away from an odd multiple of pi (`make_case` moves psi where it is not), far more than E_d.
    E_phi, one neighbour: E_at + u |psi difference| + u |phi|;  whole row: 0 (phi is psi's bits).
    E_mag: rel_As = mel ? (u + 2^-22 |L|) / 2 + 2^-22 : 0, L = log(max(a, 0) + eps) (the sum's rounding, logf and expf
              within 2 ulp); w == 1: As rel_As; else mag (E_arg + 2^-22),
              E_arg = (1 - w) (3u + 2^-22 |log Ao|) + 2u (1 - w) |log Ao| + w (rel_As + 2^-22 |log As|) + u w |log As| + u |arg|
              (Ao from two products, a sum and a correctly rounded root: 3u; 1 - w and the two products round once each).
An element with bound 0 (a silent side) must be 0.

The blend: g[n] = sum of w_k^2 over the touched frames that reach n / the same sum over all frames of [0, T_frames) that reach
n, w the periodic Hann window, k = n + n_fft - hop - t hop, a frame reaches n when 0 < k < n_fft (w_0 = 0).  out = orig bit for
bit where g == 0, else orig + g (ola - orig); g is exactly 1 where every reaching frame is touched (the two sums are then the
same sum).  Bound: |ola - orig| E_g + u (3 g |ola - orig| + |out|), E_g = 0 where g is 0 or 1, else 2 S / den + 2u with
S = sum over reaching frames of (2 w_k dw + dw^2 + u w_k^2) + m u den, dw = 2^-20 (cosf within 2 ulp of its value, its
argument k float32(2 pi) / n_fft within 3u 2 pi, halved, one more rounding), m the number of reaching frames."""
import math
from types import SimpleNamespace

import numpy as np

PI = math.pi
U = 2.0 ** -24
EPS32 = float(np.float32(1e-6))
E_AT = 2.0 ** -21
WRAP_MARGIN = 1e-2
OUT_POISON = 0x7FC5A5A5          # a NaN no kernel makes
MUTANTS = ("no_detune", "anchor_at_t0", "no_wrap", "run_end_off_by_one", "right_sign", "linear_magnitude", "copy_recomputed")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def wrap(d):
    """principal value in (-pi, pi]"""
    d = np.asarray(d)
    two_pi, pi = d.dtype.type(2.0 * PI), d.dtype.type(PI)
    return d - two_pi * np.ceil((d - pi) / two_pi)


def runs(mask):
    """mask bool [B, T, F] -> (t0, t1) int64 [B, T, F]: the run [t0, t1) of every frame inside one (anything elsewhere)"""
    T = mask.shape[1]
    idx = np.arange(T, dtype=np.int64)[None, :, None]
    prev = np.concatenate([np.zeros_like(mask[:, :1]), mask[:, :-1]], 1)
    t0 = np.maximum.accumulate(np.where(mask & ~prev, idx, -1), axis=1)
    t1 = np.minimum.accumulate(np.where(~mask, idx, T)[:, ::-1], axis=1)[:, ::-1]
    return t0, t1


def synthesis_magnitude(a, mel, dtype=np.float64):
    a = np.asarray(a, dtype=dtype)
    if not mel:
        return a
    return np.exp(dtype(0.5) * np.log(np.maximum(a, dtype(0.0)) + dtype(EPS32)))


def splice(xo, a, ph, w, mel, dtype=np.float64, mutant=None):
    """The specification (dtype float64) or its float32 model in the kernel's order (dtype float32; `mutant`: one of MUTANTS).
    Returns a namespace: out complex [B, T, F] (float64) or float [B, T, 2F] (float32), and, for float64, the masks and the
    bound's parts."""
    xo32 = np.asarray(xo, dtype=np.float32)
    B, T, F2 = xo32.shape
    F = F2 // 2
    re, im = xo32[..., :F].astype(dtype), xo32[..., F:].astype(dtype)
    psi = np.asarray(ph, dtype=np.float32).astype(dtype)
    wb = np.broadcast_to(np.asarray(w, dtype=np.float32), (B, T, F)).astype(dtype)
    mask = wb > 0
    t0, t1 = runs(mask)
    left, right = t0 >= 1, t1 <= T - 1
    both, whole = left & right, ~left & ~right
    ia = np.clip(t0 if mutant == "anchor_at_t0" else t0 - 1, 0, T - 1)
    ib = np.clip(t1 + 1 if mutant == "run_end_off_by_one" else t1, 0, T - 1)
    phio = np.arctan2(im, re)
    take = lambda x, i: np.take_along_axis(x, i, axis=1)                                   # noqa: E731
    phia, psia, phib, psib = take(phio, ia), take(psi, ia), take(phio, ib), take(psi, ib)
    n1 = (t1 - t0 + 1).astype(dtype)
    j = (np.arange(T, dtype=np.int64)[None, :, None] - t0 + 1).astype(dtype)
    d = (phib - phia) - (psib - psia)
    c = (d if mutant == "no_wrap" else wrap(d)) / n1
    if mutant == "no_detune":
        c = np.zeros_like(c)
    phi_both = (phia + (psi - psia)) + j * c
    phi_left = phia + (psi - psia)
    phi_right = phib + (psib - psi) if mutant == "right_sign" else phib - (psib - psi)
    phi = np.where(both, phi_both, np.where(left, phi_left, np.where(right, phi_right, psi)))
    As = synthesis_magnitude(a, mel, dtype)
    Ao = np.sqrt(re * re + im * im)
    live = (Ao > 0) & (As > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo, ls = np.log(np.where(live, Ao, 1)), np.log(np.where(live, As, 1))
        arg = (dtype(1.0) - wb) * lo + wb * ls
        blend = (dtype(1.0) - wb) * Ao + wb * As if mutant == "linear_magnitude" else np.exp(arg)
    mag = np.where(wb == 1, As, np.where(live, blend, dtype(0.0)))
    if dtype == np.float32:
        o_re, o_im = np.where(mask, mag * np.cos(phi), re), np.where(mask, mag * np.sin(phi), im)
        if mutant == "copy_recomputed":
            o_re, o_im = np.where(mask, o_re, Ao * np.cos(phio)), np.where(mask, o_im, Ao * np.sin(phio))
        return SimpleNamespace(out=np.concatenate([o_re, o_im], -1).astype(np.float32))

    out = np.where(mask, mag * np.exp(1j * phi), re + 1j * im)
    # ---- the bound
    e_d = 2 * E_AT + U * np.abs(phib - phia) + U * np.abs(psib - psia) + U * np.abs(d) + 4 * U * (np.abs(d) + 2 * PI)
    e_c = e_d / n1 + U * np.abs(c)
    e_both = E_AT + U * np.abs(psi - psia) + U * np.abs(phia + (psi - psia)) + j * e_c + U * np.abs(j * c) + U * np.abs(phi)
    e_left = E_AT + U * np.abs(psi - psia) + U * np.abs(phi)
    e_right = E_AT + U * np.abs(psib - psi) + U * np.abs(phi)
    e_phi = np.where(both, e_both, np.where(left, e_left, np.where(right, e_right, 0.0)))
    e_phase = e_phi + 1.5 * 2.0 ** -22 + 2 * U
    if mel:
        L = np.log(np.maximum(np.asarray(a, dtype=np.float32).astype(np.float64), 0.0) + EPS32)
        rel_as = 0.5 * (U + 2.0 ** -22 * np.abs(L)) + 2.0 ** -22
    else:
        rel_as = np.zeros_like(As)
    e_arg = ((1 - wb) * (3 * U + 2.0 ** -22 * np.abs(lo)) + 2 * U * (1 - wb) * np.abs(lo)
             + wb * (rel_as + 2.0 ** -22 * np.abs(ls)) + U * wb * np.abs(ls) + U * np.abs(arg))
    e_mag = np.where(wb == 1, As * rel_as, mag * (e_arg + 2.0 ** -22))
    bound = np.where(mask, np.abs(mag) * e_phase + e_mag, 0.0)
    margin = np.where(mask & both, np.abs(PI - np.abs(wrap(d))), np.inf)
    return SimpleNamespace(out=out, bound=bound, mask=mask, exact=mask & whole & (wb == 1), both=both, left=left, right=right,
                           t0=t0, t1=t1, c=np.where(mask & both, c, 0.0), phi=phi, mag=mag, margin=margin)


def to_stft_f32_model(a, ph, mel):
    """isi_spec_to_stft_f32 in float32 numpy: what a whole-row run at w == 1 is compared with where no GPU ran the kernel"""
    mag = synthesis_magnitude(a, mel, np.float32)
    ph = np.asarray(ph, dtype=np.float32)
    return np.concatenate([mag * np.cos(ph), mag * np.sin(ph)], -1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the cases
KERNEL_F, KERNEL_T, KERNEL_B = (1, 5, 64, 130), (1, 2, 3, 17, 40), (1, 3)
N_PATTERNS = 8


def weight_row(p, T, k, g):
    """one (w_batch, k) row of weights: the patterns the issue lists"""
    w = np.zeros(T)
    if p == 1:                                         # the whole row, regenerated
        w[:] = 1.0
    elif p == 2:                                       # the whole row, fractional
        w[:] = g.uniform(0.05, 0.95, T)
    elif p == 3:                                       # a run at frame 0 (the whole row when T == 1)
        w[:1 + k % max(1, T - 1)] = 1.0
    elif p == 4:                                       # a run that ends at T
        w[T - 1 - k % max(1, T - 1):] = 1.0
    elif p == 5:                                       # runs of one frame, one frame apart
        w[1::2] = 1.0
    elif p == 6:                                       # several runs, fractional and whole weights
        on = g.uniform(size=T) < 0.5
        w[on] = np.where(g.uniform(size=int(on.sum())) < 0.5, 1.0, g.uniform(0.05, 0.95, int(on.sum())))
    elif p == 7 and T >= 3:                            # an interior run with ramps
        n = T - 2
        w[1:T - 1] = np.minimum(1.0, np.minimum(np.arange(1, n + 1), np.arange(n, 0, -1)) / 3.0)
    return w


def make_case(B, T, F, w_batch, mel, seed=0):
    g = np.random.default_rng([B, T, F, w_batch, mel, seed])
    xo = (g.standard_normal((B, T, 2 * F)) * np.exp(g.standard_normal((B, T, 2 * F)))).astype(np.float32)
    if mel:
        a = g.standard_normal((B, T, F)) ** 2
        a[g.uniform(size=a.shape) < 0.02] = -1e-3      # a negative power: clamped
    else:
        a = np.exp(g.standard_normal((B, T, F)))
    a = a.astype(np.float32)
    psi = g.uniform(-30 * PI, 30 * PI, (B, 1, F)) + np.cumsum(g.uniform(-PI, PI, (B, T, F)), 1)
    psi *= 40 * PI / np.abs(psi).max()                 # the largest |psi| of the case is 40 pi
    w = np.zeros((w_batch, T, F))
    for wb in range(w_batch):
        for k in range(F):
            w[wb, :, k] = weight_row((k + wb + seed + T) % N_PATTERNS, T, k, g)
    w = w.astype(np.float32)
    silent = (np.arange(F) + seed + T) % N_PATTERNS == 2          # silent original bins under (row 0's) fractional weights
    xo[:, T // 2, np.concatenate([silent, silent])] = 0.0
    ph = psi.astype(np.float32)
    for _ in range(20):                                # keep every wrap decision WRAP_MARGIN from flipping
        s = splice(xo, a, ph, w, mel)
        tie = np.argwhere(s.margin < WRAP_MARGIN)
        if not len(tie):
            break
        b, t, k = tie[0]
        ph[b, s.t1[b, t, k]:, k] += np.float32(0.37)
    else:
        raise AssertionError("wrap ties remain")
    s = splice(xo, a, ph, w, mel)
    return SimpleNamespace(B=B, T=T, F=F, w_batch=w_batch, mel=mel, xo=xo, a=a, ph=ph, w=w, spec=s,
                           name=f"B={B} T={T} F={F} w_batch={w_batch} mel={mel}")


def kernel_cases(T, F):
    for B in KERNEL_B:
        for w_batch in sorted({1, B}):
            for mel in (0, 1):
                yield make_case(B, T, F, w_batch, mel)


def compare(got, case, what=None, exact_ref=None):
    """got float32 [B, T, 2F] against the case's specification; returns the worst error / bound.  Copied elements bit for bit
    against the original; whole-row runs at w == 1 bit for bit against `exact_ref` (isi_spec_to_stft_f32's output, or its
    model) when given."""
    what = what or case.name
    s, F = case.spec, case.F
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == case.xo.shape, f"{what}: shape {got.shape}"
    copied = np.concatenate([~s.mask, ~s.mask], -1)
    assert np.array_equal(bits(got)[copied], bits(case.xo)[copied]), f"{what}: an element with w == 0 is not the original's bits"
    if exact_ref is not None:
        exact = np.concatenate([s.exact, s.exact], -1)
        assert np.array_equal(bits(got)[exact], bits(exact_ref)[exact]), \
            f"{what}: a whole-row run at w == 1 is not isi_spec_to_stft_f32's bits"
    z = got[..., :F].astype(np.float64) + 1j * got[..., F:].astype(np.float64)
    assert np.isfinite(z[s.mask]).all(), f"{what}: a regenerated element is not finite"
    err = np.abs(z - s.out)
    zero = s.mask & (s.bound == 0)
    assert not (err[zero] != 0).any(), f"{what}: an element with a silent side is not 0"
    live = s.mask & (s.bound > 0)
    ratio = float((err[live] / s.bound[live]).max()) if live.any() else 0.0
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    return ratio


# ------------------------------------------------------------------------------------------------------------- the blend
def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * PI * np.arange(n_fft) / n_fft)


def blend(orig, ola, touched, n_fft, hop):
    """float64 specification of isi_spec_splice_blend_f32: namespace(out, g, bound, copied, full)"""
    o, s = np.asarray(orig, dtype=np.float32).astype(np.float64), np.asarray(ola, dtype=np.float32).astype(np.float64)
    touched = np.asarray(touched) != 0
    (B, L), Tf = o.shape, touched.shape[1]
    pos = np.arange(L) + n_fft - hop
    win, dw = hann(n_fft), 2.0 ** -20
    num, den, S = np.zeros((B, L)), np.zeros(L), np.zeros(L)
    reach, hit = np.zeros(L, dtype=np.int64), np.zeros((B, L), dtype=np.int64)
    for t in range(Tf):
        k = pos - t * hop
        valid = (k > 0) & (k < n_fft)
        wk = np.where(valid, win[np.clip(k, 0, n_fft - 1)], 0.0)
        den += wk * wk
        S += np.where(valid, 2 * wk * dw + dw * dw + U * wk * wk, 0.0)
        reach += valid
        num += touched[:, t, None] * (wk * wk)[None]
        hit += touched[:, t, None] & valid[None]
    copied, full = hit == 0, (hit == reach[None]) & (reach[None] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(copied, 0.0, np.where(full, 1.0, num / den[None]))
        e_g = np.where(copied | full, 0.0, 2 * (S + reach * U * den)[None] / den[None] + 2 * U)
    out = np.where(copied, o, o + g * (s - o))
    bound = np.abs(s - o) * e_g + U * (3 * g * np.abs(s - o) + np.abs(out))
    return SimpleNamespace(out=out, g=g, bound=bound, copied=copied, full=full)


def blend_f32_model(orig, ola, touched, n_fft, hop):
    """the kernel's order in float32"""
    o, s = np.asarray(orig, dtype=np.float32), np.asarray(ola, dtype=np.float32)
    touched = np.asarray(touched) != 0
    (B, L), Tf = o.shape, touched.shape[1]
    pos = np.arange(L) + n_fft - hop
    step = np.float32(2.0 * PI) / np.float32(n_fft)
    num, den = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    for t in range(Tf - 1, -1, -1):
        k = pos - t * hop
        valid = (k >= 0) & (k < n_fft)
        wk = np.float32(0.5) - np.float32(0.5) * np.cos(k.astype(np.float32) * step)
        w2 = np.where(valid, wk * wk, np.float32(0)).astype(np.float32)
        den = den + w2[None]
        num = num + np.where(touched[:, t, None], w2[None], np.float32(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(num != 0, o + (num / den) * (s - o), o).astype(np.float32)


BLEND_GEOMETRIES = [(16, 4, 9, 24), (256, 64, 11, 512), (64, 64, 5, 320), (64, 32, 7, 200), (256, 64, 1, 64)]   # n_fft, hop, T_frames, L


def make_blend_case(n_fft, hop, Tf, L, B, seed=0):
    g = np.random.default_rng([n_fft, hop, Tf, L, B, seed])
    orig, ola = g.standard_normal((B, L)).astype(np.float32), g.standard_normal((B, L)).astype(np.float32)
    touched = np.zeros((B, Tf), dtype=np.uint8)
    for b in range(B):
        if b % 3 == 0 and Tf >= 3:
            touched[b, Tf // 3:2 * Tf // 3 + 1] = 1            # an interior hole
        elif b % 3 == 1:
            touched[b] = g.uniform(size=Tf) < 0.4               # scattered frames
            touched[b, 0] = 7                                   # any non-zero byte counts
        # b % 3 == 2: untouched
    if B == 1 and Tf < 3:
        touched[:] = 1
    return SimpleNamespace(n_fft=n_fft, hop=hop, Tf=Tf, L=L, B=B, orig=orig, ola=ola, touched=touched,
                           spec=blend(orig, ola, touched, n_fft, hop), name=f"n_fft={n_fft} hop={hop} T_frames={Tf} L={L} B={B}")


def compare_blend(got, case, what=None):
    what, s = what or case.name, case.spec
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == case.orig.shape
    assert np.array_equal(bits(got)[s.copied], bits(case.orig)[s.copied]), f"{what}: a sample no touched frame reaches is not the original's bits"
    err = np.abs(got.astype(np.float64) - s.out)
    ratio = float((err[~s.copied] / s.bound[~s.copied]).max()) if (~s.copied).any() else 0.0
    assert ratio <= 1.0, f"{what}: error / bound = {ratio:.3f}"
    return ratio


# -------------------------------------------------------------------------- the helper's STFT pair in float64, the experiment
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
    """complex [T, F] -> the kernels' [1, T, 2F]"""
    return np.concatenate([X.real, X.imag], -1)[None].astype(np.float32)


def experiment_signal(T=64, n_fft=256, hop=64, hole=(25, 39), jitter=0.02, seed=0):
    """Three stationary partials (peak 1.75) and a `decoded` (a, psi) of them: the true magnitudes, the true instantaneous
    frequency plus `jitter` rad of noise per frame, integrated from a random start phase.  Returns a namespace with the
    float32 arrays the kernels take (T + n_fft / hop - 1 frames of the zero-padded original among them)."""
    g = np.random.default_rng(seed)
    L, F, extra = T * hop, n_fft // 2, n_fft // hop - 1
    n = np.arange(L)
    x = sum(amp * np.cos(2 * PI * f * n / n_fft + g.uniform(0, 2 * PI)) for amp, f in ((1.0, 9.3), (0.5, 23.71), (0.25, 51.4)))
    Xo = stft(x, n_fft, hop, T + extra)
    phio = np.angle(Xo[:T])
    IF = np.concatenate([g.uniform(-PI, PI, (1, F)), wrap(np.diff(phio, axis=0))], 0) + jitter * g.standard_normal((T, F))
    w = np.zeros((1, T, F), dtype=np.float32)
    w[:, hole[0]:hole[1]] = 1.0
    touched = np.zeros((1, T + extra), dtype=np.uint8)
    touched[:, hole[0]:hole[1]] = 1
    return SimpleNamespace(T=T, n_fft=n_fft, hop=hop, L=L, F=F, extra=extra, hole=hole, audio=x.astype(np.float32), Xo=Xo,
                           xo=pack(Xo[:T]), a=np.abs(Xo[:T])[None].astype(np.float32), ph=np.cumsum(IF, 0)[None].astype(np.float32),
                           w=w, touched=touched)


def experiment_rms(e, spliced, naive):
    """rms difference from the original over the samples every frame of which lies in the hole (g == 1), for two [L] signals"""
    inside = blend(e.audio[None], e.audio[None], e.touched, e.n_fft, e.hop).full[0]
    x = e.audio.astype(np.float64)
    rms = lambda y: float(np.sqrt(np.mean((np.asarray(y, dtype=np.float64)[inside] - x[inside]) ** 2)))      # noqa: E731
    return rms(spliced), rms(naive)


def experiment(seed=0, **kw):
    """the float64 experiment: (rms of the locked splice, rms of the naive splice, largest |c|)"""
    e = experiment_signal(seed=seed, **kw)
    s = splice(e.xo, e.a, e.ph, e.w, 0)
    naive_frames = np.where(e.w[0] > 0, e.a[0].astype(np.float64) * np.exp(1j * e.ph[0].astype(np.float64)), e.Xo[:e.T])
    sounds = []
    for frames in (s.out[0], naive_frames):
        ola = istft(np.concatenate([frames, e.Xo[e.T:]], 0), e.n_fft, e.hop, e.L)
        sounds.append(blend(e.audio[None], ola[None].astype(np.float32), e.touched, e.n_fft, e.hop).out[0])
    locked, naive = experiment_rms(e, *sounds)
    return locked, naive, float(np.abs(s.c).max())
