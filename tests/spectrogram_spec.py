"""Float64 specifications of the kernels of csrc/spectrogram.hip, the float32 yardsticks of the same operations, the cases of
tests/test_spectrogram_kernels_gpu.py with their data, and the rules that file holds each kernel to.  Plain torch on the CPU:
no GPU and none of the project's kernels.  tests/test_spectrogram_kernels_host.py holds the specifications to
oracle/spectrogram_oracle.py and to float64 autograd, and shows what each rule accepts and rejects.

Layouts, as include/isi_hip.h documents them:
    stft  [B, T, 2F]   real block | imaginary block            a, ph [B, T, F]
    spec  [B, 2, F, T] channel 0 log-magnitude, channel 1 instantaneous frequency in units of pi
    frames [B, T, n_fft], audio [B, L];  xp, xt, dx [B, T, RS] with RS >= 2F;  partial [B, ceil(T / rows_per_block), 4]
    affine: x, ref, y [B, 2, HW]

A specification takes the kernel's own float32 inputs, converts them to float64 and evaluates the closed form with math.pi.
A yardstick is the same formula in float32 torch; every running sum in one is an explicit sequential loop over t (float32
torch.cumsum sums pairwise and is more accurate than the sequential sum a kernel performs, so it would not price one).
The keyword switches of the yardsticks are the host tests' mutants: each imitates a way a kernel could be wrong.

Two kinds of rule:
  rows_check   tests_support.compare_rows, margin 8, floor 2^-23, rows = the unit-stride dimension of the output;
  bound_check  |got - spec| <= bound element by element, for the sums whose rounding has an order-free bound:
      running sums   |err_t| <= (n_t + 2) 2^-24 sum |terms|: n_t terms pi x_s summed into output t; a sum of n terms rounds
                     n - 1 times, each by at most 2^-24 of a partial sum that is at most sum |terms|; the + 2 covers the
                     rounded product and float32(pi) (0.47 x 2^-24 from pi), plus the headroom of one more rounding;
      overlap-add    |err_n| <= (m_n + 1) 2^-24 sum |terms|, m_n the number of frames that reach sample n."""
import collections
import math

import torch

import tests_support as TS

EPS = 1e-6
PI = math.pi
U24 = 2.0 ** -24
F64, F32 = torch.float64, torch.float32


def _t(x, dtype):
    return torch.as_tensor(x).detach().cpu().to(dtype)


# ------------------------------------------------------------------------------------------------------------- wrap
def wrap(d):
    """Principal value of d in [-pi, pi], float64, with the convention of oracle.spectrogram_oracle.wrap (numpy.unwrap's):
    an odd multiple of pi maps to +pi for d > 0 and to -pi for d < 0.  Written as d - 2 pi k, k = ceil((d - pi) / 2 pi)."""
    d = _t(d, F64)
    w = d - 2.0 * PI * torch.ceil((d - PI) / (2.0 * PI))            # (-pi, pi]
    return torch.where((w == PI) & (d < 0), torch.full_like(w, -PI), w)


def wrap_f32(d, end_convention=True):
    """The oracle's formula in float32.  Mutant: `end_convention` False leaves -pi where d > 0 asks for +pi."""
    pi = torch.tensor(PI, dtype=F32)
    w = torch.remainder(d + pi, 2 * pi) - pi
    if end_convention:
        w = torch.where((w == -pi) & (d > 0), pi.expand_as(w), w)
    return w


def wrap_margin(d):
    """Smallest distance of the raw differences d (float64) from an odd multiple of pi: how far every decision of `wrap` is
    from flipping."""
    r = torch.remainder(_t(d, F64) - PI, 2.0 * PI)
    return float(torch.minimum(r, 2.0 * PI - r).min()) if r.numel() else math.inf


# -------------------------------------------------------------------------------------------------- forward front-end
def _polar(stft, mel, dtype, wrapf):
    x = _t(stft, dtype)
    F = x.shape[-1] // 2
    re, im = x[..., :F], x[..., F:]
    ang = torch.atan2(im, re)
    if not mel:
        return torch.log(torch.sqrt(re * re + im * im) + EPS), ang
    ph = ang.clone()
    for t in range(1, x.shape[1]):                                  # running sum of the wrapped differences
        ph[:, t] = ph[:, t - 1] + wrapf(ang[:, t] - ang[:, t - 1])
    return re * re + im * im, ph


def polar(stft, mel):
    """stft [B,T,2F] -> (a, ph) [B,T,F].  mel 0: a = log(|X| + 1e-6), ph = angle(X) = atan2(im, re); mel 1: a = |X|^2,
    ph[0] = angle[0], ph[t] = ph[t-1] + wrap(angle[t] - angle[t-1])."""
    return _polar(stft, mel, F64, wrap)


def polar_f32(stft, mel):
    return _polar(stft, mel, F32, wrap_f32)


def polar_raw_differences(stft):
    """The differences angle[t] - angle[t-1] (float64) that the mel mode wraps."""
    x = _t(stft, F64)
    F = x.shape[-1] // 2
    ang = torch.atan2(x[..., F:], x[..., :F])
    return ang[:, 1:] - ang[:, :-1]


def _finish(a, ph, mel, dtype, wrapf, pi, first_differenced=False, forward_difference=False):
    a, ph = _t(a, dtype), _t(ph, dtype)
    T = ph.shape[1]
    c0 = torch.log(a + EPS) if mel else a
    d = ph.clone()
    if forward_difference:
        nxt = torch.cat([ph[:, 1:], ph[:, -1:]], 1)
        d[:, 1:] = wrapf(nxt[:, 1:] - ph[:, 1:])
    elif T > 1:
        d[:, 1:] = wrapf(ph[:, 1:] - ph[:, :-1])
    if first_differenced:
        d[:, 0] = wrapf(ph[:, 0])
    return torch.stack([c0, d / pi], 1).transpose(2, 3).contiguous()


def finish(a, ph, mel):
    """a, ph [B,T,F] -> spec [B,2,F,T]: channel 0 = mel ? log(a + 1e-6) : a; channel 1 = the first frame's phase kept, every
    later frame wrap(ph[t] - ph[t-1]), all divided by pi."""
    return _finish(a, ph, mel, F64, wrap, PI)


def finish_f32(a, ph, mel, end_convention=True, first_differenced=False, forward_difference=False):
    """Mutants: `end_convention` (see wrap_f32); `first_differenced`: the first frame wrapped as a difference from 0
    instead of kept; `forward_difference`: ph[t+1] - ph[t] in place of ph[t] - ph[t-1]."""
    return _finish(a, ph, mel, F32, lambda d: wrap_f32(d, end_convention), torch.tensor(PI, dtype=F32), first_differenced,
                   forward_difference)


def finish_raw_differences(ph):
    ph = _t(ph, F64)
    return ph[:, 1:] - ph[:, :-1]


# -------------------------------------------------------------------------------------------------- inverse front-end
def _neighbour(run):
    """run[..., f] <- run[..., f ^ 1] (the last of an odd count keeps its own)."""
    F = run.shape[-1]
    idx = torch.arange(F) ^ 1
    idx[idx >= F] = F - 1
    return run[..., idx]


def _inverse_prepare(spec, dtype, pi, drop_carry_at=None, share_carry=False):
    s = _t(spec, dtype)
    B, _, F, T = s.shape
    a = torch.exp(s[:, 0]).transpose(1, 2).contiguous()
    x = s[:, 1].transpose(1, 2)                                      # [B,T,F]
    ph = torch.empty(B, T, F, dtype=dtype)
    run = torch.zeros(B, F, dtype=dtype)
    for t in range(T):
        if drop_carry_at is not None and t == drop_carry_at:
            run = torch.zeros_like(run)
        if share_carry and t and t % 32 == 0:
            run = _neighbour(run)
        run = run + x[:, t] * pi
        ph[:, t] = run
    return a, ph


def inverse_prepare(spec):
    """spec [B,2,F,T] -> (a, ph) [B,T,F]: a = exp(ch0), ph[t] = sum over s <= t of pi ch1[s]."""
    return _inverse_prepare(spec, F64, PI)


def inverse_prepare_f32(spec, drop_carry_at=None, share_carry=False):
    """Mutants: `drop_carry_at`: the running sum restarts at that frame (a tile's carry lost); `share_carry`: at every
    32-frame tile edge a frequency continues from its neighbour's sum."""
    return _inverse_prepare(spec, F32, torch.tensor(PI, dtype=F32), drop_carry_at, share_carry)


def inverse_prepare_bound(spec):
    """[B,T,F]: (n_t + 2) 2^-24 sum_{s <= t} |pi ch1[s]|, n_t = t + 1."""
    x = _t(spec, F64)[:, 1].transpose(1, 2).abs() * PI
    n = torch.arange(1, x.shape[1] + 1, dtype=F64).view(1, -1, 1)
    return (n + 2.0) * U24 * torch.cumsum(x, 1)


def _to_stft(a, ph, mel, dtype, clamp=True):
    a, ph = _t(a, dtype), _t(ph, dtype)
    mag = a
    if mel:                                                          # the oracle's form of sqrt: exp(log / 2)
        mag = torch.exp(0.5 * torch.log((a.clamp(min=0.0) if clamp else a) + EPS))
    return torch.cat([mag * torch.cos(ph), mag * torch.sin(ph)], -1)


def to_stft(a, ph, mel):
    """a, ph [..., F] -> stft [..., 2F] = mag (cos ph | sin ph), mag = mel ? sqrt(max(a, 0) + 1e-6) : a."""
    return _to_stft(a, ph, mel, F64)


def to_stft_f32(a, ph, mel, clamp=True):
    """Mutant: `clamp` False takes sqrt(a + eps) of a negative power."""
    return _to_stft(a, ph, mel, F32, clamp)


def overlap_add(frames, hop, left, L, dtype=F64, with_bound=False, t_hi_off=0, break_past=False, ignore_left=False):
    """audio[b, n] = sum over t of frames[b, t, left + n - t hop], over the t with 0 <= left + n - t hop < n_fft: the
    literal sum, zero where no frame reaches.  with_bound: also (m_n + 1) 2^-24 sum |terms| in float64.
    Mutants (each restates the window of the kernel's loop `for t = t_hi .. 0: k = pos - t hop; if k >= n_fft break`):
    `t_hi_off` -1: the loop starts one frame early (k >= hop only); `break_past`: the break at k > n_fft, so k = n_fft is
    read -- in memory the first sample of the next frame, NaN past the last; `ignore_left`: pos = n."""
    fr = _t(frames, dtype)
    B, T, n_fft = fr.shape
    flat = torch.cat([fr.reshape(B * T * n_fft), torch.full((n_fft,), math.nan, dtype=dtype)])
    pos = torch.arange(L) + (0 if ignore_left else left)
    out = torch.zeros(B, L, dtype=dtype)
    mass, count = torch.zeros(B, L, dtype=F64), torch.zeros(L, dtype=F64)
    base = (torch.arange(B) * T * n_fft).view(B, 1)
    for t in range(T):
        k = pos - t * hop
        valid = (k >= (hop if t_hi_off < 0 else 0)) & ((k <= n_fft) if break_past else (k < n_fft))
        term = flat[base + t * n_fft + k.clamp(0, n_fft).view(1, L)]
        term = torch.where(valid.view(1, L), term, torch.zeros_like(term))
        out = out + term
        mass += term.double().abs()
        count += valid.double()
    return (out, (count + 1.0) * U24 * mass) if with_bound else out


# --------------------------------------------------------------------------------------------------------- adjoints
def _to_stft_bwd(a, ph, dx, mel, dtype):
    a, ph, dx = _t(a, dtype), _t(ph, dtype), _t(dx, dtype)
    F = a.shape[-1]
    gr, gi = dx[..., :F], dx[..., F:]
    mag, dmag = a, torch.ones_like(a)
    if mel:
        pw = a.clamp(min=0.0) + EPS
        mag = torch.exp(0.5 * torch.log(pw))
        dmag = torch.where(a > 0, 0.5 * mag / pw, torch.zeros_like(a))
    cs, sn = torch.cos(ph), torch.sin(ph)
    return (gr * cs + gi * sn) * dmag, mag * (gi * cs - gr * sn)


def to_stft_bwd(a, ph, dx, mel):
    """(da, dph) for the upstream gradient dx [..., 2F] of to_stft: da = (gr cos ph + gi sin ph) d mag / d a,
    dph = mag (gi cos ph - gr sin ph).  In mel mode mag = sqrt(max(a, 0) + eps): d mag / d a = 1 / (2 mag) for a > 0 and 0 for
    a <= 0 -- the kernel's documented choice at the kink a = 0 (the clamp's one-sided derivatives are 0 and 1 / (2 sqrt eps))."""
    return _to_stft_bwd(a, ph, dx, mel, F64)


def to_stft_bwd_f32(a, ph, dx, mel):
    return _to_stft_bwd(a, ph, dx, mel, F32)


def _inverse_prepare_bwd(spec, da, dph, dtype, pi, drop_carry_at=None, share_carry=False):
    s, da, dph = _t(spec, dtype), _t(da, dtype), _t(dph, dtype)
    B, _, F, T = s.shape
    d0 = da.transpose(1, 2) * torch.exp(s[:, 0])
    d1 = torch.empty(B, T, F, dtype=dtype)
    run = torch.zeros(B, F, dtype=dtype)
    for t in range(T - 1, -1, -1):
        if drop_carry_at is not None and t == drop_carry_at - 1:
            run = torch.zeros_like(run)
        if share_carry and t % 32 == 31:
            run = _neighbour(run)
        run = run + dph[:, t]
        d1[:, t] = run
    return torch.stack([d0, (d1 * pi).transpose(1, 2)], 1).contiguous()


def inverse_prepare_bwd(spec, da, dph):
    """d spec [B,2,F,T] from da, dph [B,T,F]: d ch0 = da exp(ch0); d ch1[t] = pi sum over s >= t of dph[s]."""
    return _inverse_prepare_bwd(spec, da, dph, F64, PI)


def inverse_prepare_bwd_f32(spec, da, dph, drop_carry_at=None, share_carry=False):
    """Mutants as inverse_prepare_f32, on the reverse scan: the sum of the frames below `drop_carry_at` restarts there."""
    return _inverse_prepare_bwd(spec, da, dph, F32, torch.tensor(PI, dtype=F32), drop_carry_at, share_carry)


def inverse_prepare_bwd_bound(dph):
    """[B,F,T]: (n_t + 2) 2^-24 sum_{s >= t} |pi dph[s]|, n_t = T - t."""
    x = _t(dph, F64).abs() * PI
    T = x.shape[1]
    n = torch.arange(T, 0, -1, dtype=F64).view(1, -1, 1)
    return ((n + 2.0) * U24 * torch.flip(torch.cumsum(torch.flip(x, [1]), 1), [1])).transpose(1, 2)


# --------------------------------------------------------------------------------------------------- spectral distance
def _distance_terms(xp, xt, F, eps, dtype, im_off=0):
    xp, xt = _t(xp, dtype), _t(xt, dtype)
    pr, pi_, tr, ti = xp[..., :F], xp[..., F - im_off:2 * F - im_off], xt[..., :F], xt[..., F - im_off:2 * F - im_off]
    mp, mt = torch.sqrt(pr * pr + pi_ * pi_), torch.sqrt(tr * tr + ti * ti)
    return pr, pi_, mp, mp - mt, torch.log(mp + eps) - torch.log(mt + eps)


def distance_sums(xp, xt, F, RS, eps, rows_per_block, dtype=F64, unclamped=False, im_off=0, drop_last=False):
    """partial [B, nchunk, 4]: per sample and chunk of rows_per_block frames (the last chunk ragged) the sums of |dm|, dm^2,
    |dl|, dl^2 over the chunk's frames and the F bins; dm = |Xp| - |Xt|, dl = log(|Xp| + eps) - log(|Xt| + eps).
    Mutants: `unclamped`: a chunk runs t0 .. t0 + rows_per_block whatever T is, into the next sample's rows (past the last
    sample: nothing); `im_off` 1: the imaginary block read at o + F - 1; `drop_last`: a chunk's last element left out."""
    assert xp.shape[-1] == RS >= 2 * F
    _, _, _, dm, dl = _distance_terms(xp, xt, F, eps, dtype, im_off)
    B, T, _ = dm.shape
    nchunk = -(-T // rows_per_block)
    v = torch.stack([dm.abs(), dm * dm, dl.abs(), dl * dl], -1).reshape(B * T, F, 4)
    out = torch.zeros(B, nchunk, 4, dtype=dtype)
    for b in range(B):
        for c in range(nchunk):
            t0 = c * rows_per_block
            t1 = t0 + rows_per_block if unclamped else min(T, t0 + rows_per_block)
            rows = v[b * T + t0:min(b * T + t1, B * T)].reshape(-1, 4)
            out[b, c] = (rows[:-1] if drop_last else rows).sum(0)
    return out


def distance_grad(xp, xt, clin, clog, F, RS, eps, kind, dtype=F64, write_padding=True):
    """dx [B,T,RS] = d / d Xp of sum_b clin[b] g(dm) + clog[b] g(dl), g' = sign (kind 0; sign(0) = 0) or identity (kind 1):
    d / d (re, im) = (clin g'(dm) + clog g'(dl) / (|Xp| + eps)) (re, im) / |Xp|, 0 where |Xp| == 0; columns >= 2F are zero.
    Mutant: `write_padding` False leaves the padding columns as they were (NaN here)."""
    assert xp.shape[-1] == RS >= 2 * F and kind in (0, 1)
    pr, pi_, mp, dm, dl = _distance_terms(xp, xt, F, eps, dtype)
    cl, cg = _t(clin, dtype).view(-1, 1, 1), _t(clog, dtype).view(-1, 1, 1)
    gm, gl = (torch.sign(dm), torch.sign(dl)) if kind == 0 else (dm, dl)
    dmag = cl * gm + cg * gl / (mp + eps)
    safe = torch.where(mp > 0, mp, torch.ones_like(mp))
    zero = torch.zeros_like(mp)
    out = torch.full(tuple(xp.shape), 0.0 if write_padding else math.nan, dtype=dtype)
    out[..., :F] = torch.where(mp > 0, dmag * pr / safe, zero)
    out[..., F:2 * F] = torch.where(mp > 0, dmag * pi_ / safe, zero)
    return out


def affine_mask(x, ref, a0, b0, a1, b1, thr, use_mask, dtype=F64, strict=False):
    """x [B,2,HW] -> y: y0 = a0 x0 + b0; y1 = a1 x1 + b1, 0 where r <= thr (use_mask), r = channel 0 of `ref` when given, else
    y0.  Mutant: `strict` masks where r < thr."""
    x = _t(x, dtype)
    y0, y1 = a0 * x[:, 0] + b0, a1 * x[:, 1] + b1
    if use_mask:
        r = _t(ref, dtype)[:, 0] if ref is not None else y0
        y1 = torch.where((r < thr) if strict else (r <= thr), torch.zeros_like(y1), y1)
    return torch.stack([y0, y1], 1)


def affine_masked(x, ref, a0, b0, thr):
    """bool [B,HW]: where the float64 spec masks the phase."""
    r = _t(ref, F64)[:, 0] if ref is not None else a0 * _t(x, F64)[:, 0] + b0
    return r <= thr


# ----------------------------------------------------------------------------------------------------------- the rules
Check = collections.namedtuple("Check", "kernel case what rule err bound ratio")       # rule: "rows" (ratio <= 8) or "bound" (<= 1)


def rows_check(kernel, case, what, got, ref, yardstick, record=None):
    """tests_support.compare_rows, unchanged; the figures go to `record` whether the comparison passes or not."""
    got = _t(got, F32)
    err = TS.row_error(got, ref)
    yard = max(TS.row_error(yardstick, ref), TS.ROW_OPS_FLOOR)
    c = Check(kernel, case, what, "rows", err, yard, err / yard)
    if record is not None:
        record.append(c)
    TS.compare_rows(got, ref, yardstick, f"{kernel} {case} {what}")
    return c


def bound_check(kernel, case, what, got, ref, bound, record=None):
    """|got - ref| <= bound at every element (a zero bound asks for the exact value); ratio = the largest err / bound."""
    got, ref, bound = _t(got, F64), _t(ref, F64), _t(bound, F64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err))
    i = int(ratio.argmax())
    c = Check(kernel, case, what, "bound", float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]), float(ratio.reshape(-1)[i]))
    if record is not None:
        record.append(c)
    assert c.ratio <= 1.0, f"{kernel} {case} {what}: error {c.err:.3e} is {c.ratio:.3g} times the derived bound {c.bound:.3e}"
    return c


def same_bits(a, b):
    a, b = _t(a, F32).contiguous(), _t(b, F32).contiguous()
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ----------------------------------------------------------------------------------------------------------- the cases
_FRAMES = (1, 2, 31, 32, 33, 64, 65, 100)
# (B, T, F).  Tiled kernels (32 x 32 tiles): every T with the ragged F = 33 (one full tile and one column), every F with
# T = 65 (two tile-to-tile carries and one frame), and B = 3 on a spread of them.
TILED_SHAPES = [(1, T, 33) for T in _FRAMES] + [(3, 65, 1), (1, 65, 31), (3, 65, 36), (1, 65, 70), (3, 33, 36), (3, 1, 31),
                                            (3, 2, 70), (3, 100, 33)]
# spec_polar_kernel: 256 bins per block, one thread per bin running over t
POLAR_SHAPES = [(1, T, 257) for T in _FRAMES] + [(3, 65, 1), (1, 65, 255), (3, 65, 300), (3, 1, 300), (3, 33, 255), (3, 100, 257)]
SCAN_LONG = (1, 1000, 4)
POLAR_CASES = [(s, m) for s in POLAR_SHAPES for m in (0, 1)]
TILED_MEL_CASES = [(s, m) for s in TILED_SHAPES for m in (0, 1)]             # finish, to_stft, to_stft_bwd
SCAN_CASES = TILED_SHAPES + [SCAN_LONG]                                      # inverse_prepare, inverse_prepare_bwd
# (n_fft, hop, left, T, L)
OLA_GEOMETRIES = [(16, 4, 12, 5, 20), (16, 4, 12, 1, 4), (256, 64, 192, 9, 576), (256, 50, 0, 7, 556), (64, 24, 0, 3, 112),
                  (2048, 240, 0, 3, 2528), (16, 4, 0, 3, 40)]
OLA_CASES = [(g, B) for g in OLA_GEOMETRIES for B in (1, 3)]
DIST_EPS = 2.0 ** -10


def _distance_cases():
    out = []
    for F in (33, 129, 1025):
        for T in (1, 7, 20):
            for rpb in (1, 3, 8, T + 5):
                if min(rpb, T) * F > 1100:                           # terms per partial
                    continue
                i = len(out)
                RS = (2 * F, (2 * F + 3) // 4 * 4, 2 * F + 8)[i % 3]
                out.append((3 if (i // 3) % 2 else 1, T, F, RS, rpb))
    return out


DIST_CASES = _distance_cases()                                               # (B, T, F, RS, rows_per_block)
DIST_GRAD_CASES = [(B, T, F, RS, kind) for B, T, F, RS, rpb in DIST_CASES if rpb == 1 for kind in (0, 1)]
# (B, HW, with ref, use_mask)
AFFINE_CASES = [((1, 3)[(i + r + m) % 2], 4 * hw4, r, m) for i, hw4 in enumerate((1, 255, 257)) for r in (0, 1) for m in (0, 1)]


def case_id(c):
    if isinstance(c, tuple):
        return "-".join(case_id(v) for v in c)
    return str(c)


def _gen(*key):
    seed = 12345
    for v in key:
        seed = (seed * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def phase_walk(B, T, F, g, big):
    """float64 [B,T,F]: a first phase in (-pi, pi) and increments +-(0.05 + U (pi - 0.1)); `big`: + 2 pi k per step, k in
    [-3, 3], and + 2 pi k0, k0 in {+-1, +-2}, on the first frame, so |ph| reaches a few hundred as mel-projected phases do."""
    u = torch.rand(B, T, F, generator=g, dtype=F64)
    sgn = torch.randint(0, 2, (B, T, F), generator=g).double() * 2.0 - 1.0
    inc = sgn * (0.05 + u * (PI - 0.1))
    inc[:, 0] = (torch.rand(B, F, generator=g, dtype=F64) * 2.0 - 1.0) * (PI - 0.05)
    if big:
        inc = inc + 2.0 * PI * torch.randint(-3, 4, (B, T, F), generator=g).double()
        k0 = torch.randint(1, 3, (B, F), generator=g).double() * (torch.randint(0, 2, (B, F), generator=g).double() * 2.0 - 1.0)
        inc[:, 0] = (torch.rand(B, F, generator=g, dtype=F64) * 2.0 - 1.0) * (PI - 0.05) + 2.0 * PI * k0
    return torch.cumsum(inc, 1)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def polar_data(case):
    """stft [B,T,2F] float32: magnitudes in [0.1, 10], phases a phase_walk; re / im formed in float64, rounded once."""
    def make():
        (B, T, F), mel = case
        g = _gen(1, B, T, F, mel)
        ang = phase_walk(B, T, F, g, False)
        mag = 0.1 * 100.0 ** torch.rand(B, T, F, generator=g, dtype=F64)
        return torch.cat([mag * torch.cos(ang), mag * torch.sin(ang)], -1).float()
    return _cached(("polar_data", case), make)


def finish_data(case):
    """(a, ph) [B,T,F] float32: a = a power in [1e-3, 10] (mel) or a log-magnitude; ph a phase_walk, `big` in the mel cases."""
    def make():
        (B, T, F), mel = case
        g = _gen(2, B, T, F, mel)
        ph = phase_walk(B, T, F, g, bool(mel)).float()
        a = (1e-3 * 1e4 ** torch.rand(B, T, F, generator=g)) if mel else torch.randn(B, T, F, generator=g) * 2.0 - 3.0
        return a, ph
    return _cached(("finish_data", case), make)


def wrap_end_data():
    """(a, ph) [1,8,3] float32 whose phase steps are exactly +P, -P, +Q, -Q, +2P, -2P, 0 with P = float32(pi) and
    Q = float32(3 P): 0, P, 0, Q, 0, 2P, 0, 0 (every subtraction x - 0 or 0 - x is exact).  Returns (a, ph, steps [7])."""
    P = torch.tensor(PI, dtype=F32)
    Q = P * 3.0
    col = torch.stack([P * 0, P, P * 0, Q, P * 0, P * 2, P * 0, P * 0])
    ph = col.view(1, 8, 1).repeat(1, 1, 3).contiguous()
    return torch.zeros(1, 8, 3), ph, col[1:] - col[:-1]


def spec_data(shape):
    """spec [B,2,F,T] float32: log-magnitudes 2 randn - 3, instantaneous frequencies uniform in (-1, 1)."""
    def make():
        B, T, F = shape
        g = _gen(3, B, T, F)
        return torch.stack([torch.randn(B, F, T, generator=g) * 2.0 - 3.0, torch.rand(B, F, T, generator=g) * 2.0 - 1.0], 1)
    return _cached(("spec_data", shape), make)


def to_stft_data(case):
    """(a, ph, dx): a = magnitudes exp(randn) (mel 0) or powers 2 randn with exact zeros (mel 1: negative, zero and positive);
    ph a phase_walk (`big` in the mel cases); dx [B,T,2F] randn."""
    def make():
        (B, T, F), mel = case
        g = _gen(4, B, T, F, mel)
        a = torch.randn(B, T, F, generator=g) * 2.0 if mel else torch.exp(torch.randn(B, T, F, generator=g))
        if mel:
            a.view(-1)[::7] = 0.0
        return a, phase_walk(B, T, F, g, bool(mel)).float(), torch.randn(B, T, 2 * F, generator=g)
    return _cached(("to_stft_data", case), make)


def grad_data(shape):
    """(da, dph) [B,T,F] randn."""
    def make():
        B, T, F = shape
        g = _gen(5, B, T, F)
        return torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)
    return _cached(("grad_data", shape), make)


def ola_noise(case):
    (n_fft, hop, left, T, L), B = case
    return _cached(("ola_noise", case), lambda: torch.randn(B, T, n_fft, generator=_gen(6, n_fft, hop, left, T, L, B)))


def ola_impulses(case):
    """[(frames, t, k)]: one non-zero element per sample (a different value each), at the first and the last frame,
    k in {0, n_fft - 1}, and one interior position."""
    (n_fft, hop, left, T, L), B = case
    out = []
    for t, k in sorted({(0, 0), (0, n_fft - 1), (T - 1, 0), (T - 1, n_fft - 1), (T // 2, n_fft // 2 + 1)}):
        fr = torch.zeros(B, T, n_fft)
        fr[:, t, k] = torch.arange(1, B + 1).float() * 1.25 + 0.5
        out.append((fr, t, k))
    return out


def _pad_nan(x, RS):
    out = torch.full((*x.shape[:-1], RS), math.nan)
    out[..., :x.shape[-1]] = x
    return out


def distance_noise(B, T, F, RS):
    """(xp, xt) [B,T,RS] float32 randn, NaN in the columns >= 2F."""
    def make():
        g = _gen(7, B, T, F, RS)
        return _pad_nan(torch.randn(B, T, 2 * F, generator=g), RS), _pad_nan(torch.randn(B, T, 2 * F, generator=g) * 0.7, RS)
    return _cached(("distance_noise", B, T, F, RS), make)


def distance_pins(case):
    """(xp, xt, owners): xt = 0 and xp = 0 (NaN padding) but bins (3, 4) at f in {0, F - 1} of the first and the last row of
    three owning chunks: (sample 0, chunk 0), (sample B // 2, the middle chunk), (sample B - 1, the ragged last chunk).
    owners = {(b, chunk): number of bins set}: sum |dm| = 5 k and sum dm^2 = 25 k there, exactly."""
    B, T, F, RS, rpb = case
    nchunk = -(-T // rpb)
    xp, xt = _pad_nan(torch.zeros(B, T, 2 * F), RS), _pad_nan(torch.zeros(B, T, 2 * F), RS)
    owners = {}
    for b, c in {(0, 0), (B // 2, nchunk // 2), (B - 1, nchunk - 1)}:
        rows = {c * rpb, min(T, (c + 1) * rpb) - 1}
        for t in rows:
            for f in (0, F - 1):
                xp[b, t, f], xp[b, t, F + f] = 3.0, 4.0
        owners[(b, c)] = 2 * len(rows)
    return xp, xt, owners


def distance_grad_data(case):
    """(xp, xt, clin, clog): xp randn; xt = xp scaled by 1 +- U(0.05, 0.9) and turned by a random angle, so |dm| >= 0.05 |Xp|
    and no sign decision hangs on rounding; then bins with Xp = 0, Xt = 0, both zero, and Xp == Xt; NaN padding."""
    def make():
        B, T, F, RS, kind = case
        g = _gen(8, B, T, F, RS, kind)
        pr, pi_ = torch.randn(B, T, F, generator=g, dtype=F64), torch.randn(B, T, F, generator=g, dtype=F64)
        s = 1.0 + (torch.randint(0, 2, (B, T, F), generator=g).double() * 2.0 - 1.0) * (0.05 + 0.85 * torch.rand(B, T, F, generator=g, dtype=F64))
        th = torch.rand(B, T, F, generator=g, dtype=F64) * 2.0 * PI
        tr, ti = s * (pr * torch.cos(th) - pi_ * torch.sin(th)), s * (pr * torch.sin(th) + pi_ * torch.cos(th))
        xp, xt = torch.cat([pr, pi_], -1).float(), torch.cat([tr, ti], -1).float()
        for j, f in enumerate(sorted({0, F - 1, F // 2, F // 3, 1})):
            what = j % 4
            for x, zero in ((xp, what in (0, 2)), (xt, what in (1, 2))):
                if zero:
                    x[:, 0, f], x[:, 0, F + f] = 0.0, 0.0
            if what == 3:
                xt[:, 0, f], xt[:, 0, F + f] = xp[:, 0, f], xp[:, 0, F + f]
        clin = (torch.rand(B, generator=g) + 0.5)
        clog = (torch.rand(B, generator=g) + 0.5) * 0.3
        return _pad_nan(xp, RS), _pad_nan(xt, RS), clin, clog
    return _cached(("distance_grad_data", case), make)


AFFINE_COEFFS = tuple(float(torch.tensor(v, dtype=F32)) for v in (0.37, -1.2, 1.7, 0.25))      # a0, b0, a1, b1 as float32 holds them
AFFINE_THR = -2.5


def affine_data(case):
    """(x, ref or None) [B,2,HW] float32.  With `ref`: every fifth ref magnitude is exactly thr, the others at least 1e-3
    from it.  Without: x0 is moved where y0 = a0 x0 + b0 would come within 1e-3 of thr (the kernel masks on its own float32
    y0, so the decision must not hang on rounding)."""
    def make():
        B, HW, with_ref, use_mask = case
        g = _gen(9, B, HW, with_ref, use_mask)
        x = torch.stack([torch.randn(B, HW, generator=g) * 4.0 - 5.0, torch.rand(B, HW, generator=g) * 2.0 - 1.0], 1)
        a0, b0 = AFFINE_COEFFS[:2]
        near = (a0 * x[:, 0].double() + b0 - AFFINE_THR).abs() < 1e-3
        x[:, 0][near] += 1.0
        ref = None
        if with_ref:
            ref = torch.stack([torch.randn(B, HW, generator=g) * 2.0 + AFFINE_THR, torch.full((B, HW), math.nan)], 1)
            r0 = ref[:, 0]
            r0[(r0.double() - AFFINE_THR).abs() < 1e-3] += 0.5
            ref[:, 0, ::5] = AFFINE_THR
        return x, ref
    return _cached(("affine_data", case), make)


# ------------------------------------------------------------------------------- one kernel's output against its rules
# Every function below takes what the kernel (or a yardstick, or a mutant) returned for a case and applies the rules the
# GPU file holds that kernel to; `record` collects the figures.
def check_polar(case, a, ph, record=None):
    (B, T, F), mel = case
    x = polar_data(case)
    if mel:
        m = wrap_margin(polar_raw_differences(x))
        assert m >= 0.01, f"polar {case_id(case)}: a raw difference lies {m:.3e} rad from an odd multiple of pi"
    ra, rp = _cached(("polar_ref", case), lambda: polar(x, mel))
    ya, yp = _cached(("polar_f32", case), lambda: polar_f32(x, mel))
    rows_check("polar", case_id(case), "a", a, ra, ya, record)
    rows_check("polar", case_id(case), "ph (running sum)" if mel else "ph", ph, rp, yp, record)


def check_finish(case, out, record=None):
    (B, T, F), mel = case
    a, ph = finish_data(case)
    m = wrap_margin(finish_raw_differences(ph))
    assert m >= 0.01, f"finish {case_id(case)}: a raw difference lies {m:.3e} rad from an odd multiple of pi"
    ref = _cached(("finish_ref", case), lambda: finish(a, ph, mel))
    yard = _cached(("finish_f32", case), lambda: finish_f32(a, ph, mel))
    out = _t(out, F32)
    rows_check("finish", case_id(case), "ch0", out[:, 0], ref[:, 0], yard[:, 0], record)
    rows_check("finish", case_id(case), "ch1", out[:, 1], ref[:, 1], yard[:, 1], record)


def check_finish_wrap_ends(out, record=None):
    """Steps of exactly +-float32(pi), +-float32(3 pi), +-2 float32(pi) and 0: the float64 spec of a float32 step next to an
    odd multiple of pi lands next to -1 or +1 on either side, so the comparison is on the circle of period 2, at 2^-20; no
    output may leave [-1, 1] by more than 2^-22; and the end convention itself, stated for float32: where the step is an odd
    multiple of float32(pi), the output has the step's sign (+pi for d > 0, numpy.unwrap's choice), within 2^-20 of +-1."""
    a, ph, steps = wrap_end_data()
    ref = finish(a, ph, 0)
    got = _t(out, F64)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    d = (got[:, 1] - ref[:, 1]).abs() % 2.0
    d = torch.minimum(d, 2.0 - d)
    c = Check("finish", "wrap-ends", "ch1 on the circle", "bound", float(d.max()), 2.0 ** -20, float(d.max()) / 2.0 ** -20)
    if record is not None:
        record.append(c)
    assert c.ratio <= 1.0, f"finish wrap-ends: {c.err:.3e} from the spec on the circle of period 2"
    assert float(got[:, 1].abs().max()) <= 1.0 + 2.0 ** -22, float(got[:, 1].abs().max())
    assert bool((got[:, 0] == 0).all())
    for t, s in enumerate(steps.tolist(), start=1):
        odd = round(abs(s) / PI) % 2 == 1
        if odd:
            v = got[0, 1, :, t] * math.copysign(1.0, s)
            assert bool((v >= 1.0 - 2.0 ** -20).all()), f"finish wrap-ends: a step of {s!r} gave {got[0, 1, :, t].tolist()}"


def check_inverse_prepare(shape, a, ph, record=None):
    spec = spec_data(shape)
    ra, rp = _cached(("ip_ref", shape), lambda: inverse_prepare(spec))
    ya, _ = _cached(("ip_f32", shape), lambda: inverse_prepare_f32(spec))
    rows_check("inverse_prepare", case_id(shape), "a = exp(ch0)", a, ra, ya, record)
    bound_check("inverse_prepare", case_id(shape), "ph (running sum)", ph, rp, inverse_prepare_bound(spec), record)


def check_to_stft(case, x, record=None):
    a, ph, _ = to_stft_data(case)
    ref = _cached(("ts_ref", case), lambda: to_stft(a, ph, case[1]))
    yard = _cached(("ts_f32", case), lambda: to_stft_f32(a, ph, case[1]))
    rows_check("to_stft", case_id(case), "stft", x, ref, yard, record)


def check_to_stft_bwd(case, da, dph, record=None):
    a, ph, dx = to_stft_data(case)
    ref = _cached(("tsb_ref", case), lambda: to_stft_bwd(a, ph, dx, case[1]))
    yard = _cached(("tsb_f32", case), lambda: to_stft_bwd_f32(a, ph, dx, case[1]))
    if case[1]:
        assert bool((_t(da, F32)[a <= 0] == 0).all()), f"to_stft_bwd {case_id(case)}: d a is not exactly 0 where a <= 0"
    rows_check("to_stft_bwd", case_id(case), "da", da, ref[0], yard[0], record)
    rows_check("to_stft_bwd", case_id(case), "dph", dph, ref[1], yard[1], record)


def check_inverse_prepare_bwd(shape, dspec, record=None):
    spec = spec_data(shape)
    da, dph = grad_data(shape)
    ref = _cached(("ipb_ref", shape), lambda: inverse_prepare_bwd(spec, da, dph))
    yard = _cached(("ipb_f32", shape), lambda: inverse_prepare_bwd_f32(spec, da, dph))
    dspec = _t(dspec, F32)
    rows_check("inverse_prepare_bwd", case_id(shape), "d ch0", dspec[:, 0], ref[:, 0], yard[:, 0], record)
    bound_check("inverse_prepare_bwd", case_id(shape), "d ch1 (reverse running sum)", dspec[:, 1], ref[:, 1],
                inverse_prepare_bwd_bound(dph), record)


def check_overlap_add_impulse(case, frames, t, k, audio):
    """One non-zero frame element: the output holds that value at n = t hop + k - left when that lies in [0, L) and is
    exactly 0 everywhere else, bit for bit."""
    (n_fft, hop, left, T, L), B = case
    want = overlap_add(frames, hop, left, L).float()
    n = t * hop + k - left
    assert int((want != 0).sum()) == (B if 0 <= n < L else 0)
    assert same_bits(audio, want), f"overlap_add {case_id(case)}: impulse at frame {t}, k = {k}"


def check_overlap_add_noise(case, audio, record=None):
    (n_fft, hop, left, T, L), B = case
    ref, bound = _cached(("ola_ref", case), lambda: overlap_add(ola_noise(case), hop, left, L, with_bound=True))
    untouched = bound == 0
    assert bool((_t(audio, F32)[untouched] == 0).all()), f"overlap_add {case_id(case)}: a sample no frame reaches is not 0"
    bound_check("overlap_add", case_id(case), "audio", audio, ref, bound, record)


def check_distance_pins(case, partial, record=None):
    B, T, F, RS, rpb = case
    xp, xt, owners = distance_pins(case)
    got = _t(partial, F32)
    ref = distance_sums(xp, xt, F, RS, DIST_EPS, rpb)
    yard = distance_sums(xp, xt, F, RS, DIST_EPS, rpb, dtype=F32)
    assert got.shape == ref.shape
    for b in range(B):
        for c in range(ref.shape[1]):
            k = owners.get((b, c), 0)
            assert got[b, c, 0] == 5.0 * k and got[b, c, 1] == 25.0 * k, \
                f"distance_fwd {case_id(case)}: chunk ({b}, {c}) holds {got[b, c].tolist()}, {k} bins of magnitude 5 are its own"
            if not k:
                assert bool((got[b, c] == 0).all()), f"distance_fwd {case_id(case)}: chunk ({b}, {c}) owns nothing: {got[b, c].tolist()}"
    for j, what in ((2, "sum |dl| of the pins"), (3, "sum dl^2 of the pins")):
        rows_check("distance_fwd", case_id(case), what, got[..., j].reshape(-1), ref[..., j].reshape(-1), yard[..., j].reshape(-1), record)


def check_distance_noise(case, partial, record=None):
    B, T, F, RS, rpb = case
    xp, xt = distance_noise(B, T, F, RS)
    ref = _cached(("dist_ref", case), lambda: distance_sums(xp, xt, F, RS, DIST_EPS, rpb))
    yard = _cached(("dist_f32", case), lambda: distance_sums(xp, xt, F, RS, DIST_EPS, rpb, dtype=F32))
    got = _t(partial, F32)
    assert got.shape == ref.shape
    for j, what in enumerate(("sum |dm|", "sum dm^2", "sum |dl|", "sum dl^2")):
        rows_check("distance_fwd", case_id(case), what, got[..., j].reshape(-1), ref[..., j].reshape(-1), yard[..., j].reshape(-1), record)


def check_distance_grad(case, dx, record=None):
    B, T, F, RS, kind = case
    xp, xt, clin, clog = distance_grad_data(case)
    ref = _cached(("dg_ref", case), lambda: distance_grad(xp, xt, clin, clog, F, RS, DIST_EPS, kind))
    yard = _cached(("dg_f32", case), lambda: distance_grad(xp, xt, clin, clog, F, RS, DIST_EPS, kind, dtype=F32))
    got = _t(dx, F32)
    assert got.shape == ref.shape
    assert bool((got[..., 2 * F:] == 0).all()) and not bool(torch.isnan(got[..., 2 * F:]).any()), \
        f"distance_bwd {case_id(case)}: the padding columns are not exactly 0"
    p, t = xp[..., :2 * F], xt[..., :2 * F]
    mp0 = (p[..., :F] == 0) & (p[..., F:] == 0)
    same = (p[..., :F] == t[..., :F]) & (p[..., F:] == t[..., F:])
    assert bool(mp0.any()) and bool((same & ~mp0).any())
    zero = torch.cat([mp0 | (same & (kind == 0))] * 2, -1)
    assert bool((got[..., :2 * F][zero] == 0).all()), f"distance_bwd {case_id(case)}: not exactly 0 where |Xp| = 0" + \
        (" or Xp == Xt" if kind == 0 else "")
    if kind == 0:                                                     # no sign decision hangs on rounding, from the spec alone
        _, _, mp, dm, dl = _distance_terms(xp, xt, F, DIST_EPS, F64)
        mt0 = (t[..., :F] == 0) & (t[..., F:] == 0)
        live = ~(same | mp0 | mt0)
        assert bool(((dm.abs() >= 1e-3 * mp) | ~live).all()) and bool(((dl.abs() >= 1e-3) | ~live).all())
    rows_check("distance_bwd", case_id(case), "dx", got, ref, yard, record)


def check_affine_mask(case, y, record=None):
    B, HW, with_ref, use_mask = case
    x, ref_in = affine_data(case)
    a0, b0, a1, b1 = AFFINE_COEFFS
    ref = affine_mask(x, ref_in, a0, b0, a1, b1, AFFINE_THR, use_mask)
    yard = affine_mask(x, ref_in, a0, b0, a1, b1, AFFINE_THR, use_mask, dtype=F32)
    got = _t(y, F32)
    if use_mask:
        masked = affine_masked(x, ref_in, a0, b0, AFFINE_THR)
        if with_ref:
            on = ref_in[:, 0] == AFFINE_THR
            assert bool(on.any()) and bool((masked[on]).all())
            assert float((ref_in[:, 0].double() - AFFINE_THR).abs()[~on].min()) >= 1e-3
        else:
            assert float((ref[:, 0] - AFFINE_THR).abs().min()) >= 1e-3
        assert bool(masked.any()) and bool((~masked).any())
        assert bool(torch.equal(got[:, 1] == 0, masked | (ref[:, 1] == 0))), \
            f"affine_mask {case_id(case)}: the phase is not 0 exactly where the spec masks"
    rows_check("affine_mask", case_id(case), "y", got, ref, yard, record)
