"""isi_formant_shift_f32 (csrc/formant.hip; include/isi_hip.h carries the definition) in numpy: the
float64 definition, a float32 model in the kernel's order, planted faults, the kernel cases with their data, the error bound
and the comparison (used by tests/test_formant_host.py and tests/test_formant_gpu.py), and the float64 experiment.  No GPU.

The operation, per frame of Y [B, T, 2F] (real block | imaginary block, bin j = DFT bin k = j + 1 of n_fft = 2F), with
n = order, I = iterations, depth and max_gain in nepers, rho = ratio clamped to [1/4, 4] (a NaN counts as 1):
  P_j = fl(fl(re re) + fl(im im)) in float32, Pmax = max P_j (NaN if any is); the frame is copied bit for bit unless
  0 < Pmax < +inf, and when rho == 1;  L_j = max(1/2 ln P_j, 1/2 ln Pmax - depth);  Lx_0 = L_0, Lx_k = L_{k-1}, k = 0 .. F;
  S(A): c_q = (1 / 2F) [A_0 + (-1)^q A_F + 2 sum_{0<k<F} A_k cos(pi q k / F)], w_q = (1 + cos(pi q / n)) / 2,
        V_k = w_0 c_0 + 2 sum_{0<q<n} w_q c_q cos(pi q k / F);
  A(0) = Lx, V(i) = S(A(i-1)), A(i) = max(Lx, V(i)), V = V(I);
  x = min(fl32(rho k), F), i = min(floor x, F - 1), f = x - i, V_x = (1 - f) V_i + f V_{i+1};
  out_j = exp(clamp(V_x - V_k, -max_gain, max_gain)) (re_j, im_j).
P, rho and x are float32 quantities BY DEFINITION (they decide the copy rule and the interpolation cell), everything else is
real arithmetic: `spec` evaluates it in float64 with float64 cosines.

The bound (`spec` computes it per frame from its own intermediates; u = 2^-24; gamma(m) = m u / (1 - m u) bounds m roundings):
  * logf within ULP_LOG = 1 ulp and expf within ULP_EXP = 1 ulp (the figures the HIP device library documents); an ulp is at
    most 2 u of the value.  L_j = 0.5 logf(P_j) (the halving is exact) and the floor 0.5 logf(Pmax) - depth (one more
    rounding):  e_L = (2 ULP_LOG + 1) u max(|Lx|, |1/2 ln Pmax|, |floor|).
  * one pass on an input with error E_A and |A| <= Amax (the spec's max |A| + E_A): the exact operator carries E_A to at most
    ||S||inf E_A (computed numerically per (F, n) in float64: the largest absolute row sum of the (F+1) x (F+1) matrix), and
    the pass's own roundings add e_round:
      - a coefficient's sum of F + 1 products: one u for the table entry, and one u per rounding on the longest path of
        the kernel's order -- ceil((F + 1) / 64) chained fmas per lane and 6 butterfly levels --, one for the factor
        m_q w_q / 2F (made in double, rounded once) and one for the product with it: gamma(D_f + 3) Amax per unit of m_q w_q,
        D_f = ceil((F + 1) / 64) + 6;  all n coefficients together reach V_k through at most W = sum_q m_q w_q of it;
      - V_k's sum of n products: one u for the table entry and n chained fmas: gamma(n + 1) sum_q |d_q|, with
        sum_q |d_q| <= sum_q m_q w_q |c_q| (the spec's) + W (E_A + gamma(D_f + 3) Amax);
    E_V(i) = ||S||inf E_A(i-1) + e_round(i), E_A(i) = max(e_L, E_V(i)) because max is 1-Lipschitz, E_A(0) = e_L.
  * env is held to E_V = E_V(I).
  * the gain: V_x by (1 - f) (one rounding), a product and an fma: E_Vx = E_V + gamma(3) (max |V| + E_V); the difference
    V_x - V_k rounds once: E_g = E_Vx + E_V + u (|V_x - V_k| + E_Vx + E_V); the clamp is 1-Lipschitz; expf and the product
    with re / im: three u.  Per element |got - spec| <= |X| g (expm1(E_g') + 3 u), E_g' = E_g (1 + 4 u) + 4 u^2 (which covers the
    cross terms of the first-order form).
Copied frames are compared bit for bit, the env row of a frame without a usable Pmax is +0.0 bit for bit.

Planted faults (FAULTS; `spec(..., fault=)` evaluates the faulty definition in float64): no iteration; max against the previous
V instead of Lx; hard lifter; the (-1)^q sign of the end term dropped; DC not taken from bin 1; gain read at k / rho; no clamp
at F; no gain clamp; no floor; a rho = 1 frame recomputed instead of copied.  The last one is invisible by construction where
the gain path is right -- exp(0) = 1 returns the input's bits --, so it is planted as the removal of the branch that copies,
which is also where a NaN ratio is made to count as 1: without it a NaN reaches the clamp and comes out as 1/4."""
import math
from functools import lru_cache

import numpy as np

PI = math.pi
U = 2.0 ** -24
ULP_LOG = 1
ULP_EXP = 1
OUT_POISON = 0x7FC5A5A5          # a NaN no kernel makes
MAX_ORDER = 256
MAX_ITERATIONS = 64
DB = math.log(10.0) / 20.0       # nepers per dB
DEPTH = 80.0 * DB
MAX_GAIN = 40.0 * DB
FAULTS = ("no_iteration", "max_against_v", "hard_lifter", "end_sign_dropped", "dc_not_from_bin_1", "gain_at_k_over_rho",
          "no_clamp_at_F", "no_gain_clamp", "no_floor", "unit_ratio_recomputed")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def gamma(m):
    return m * U / (1.0 - m * U)


def cos_table64(F):
    """cos(pi i / F), i = 0 .. 2F - 1, float64; the entries at 0, F / 2, F and 3F / 2 are exact"""
    i = np.arange(2 * F)
    c = np.cos(PI * i / F)
    c[0], c[F] = 1.0, -1.0
    if F % 2 == 0:
        c[F // 2] = c[3 * F // 2] = 0.0
    return c


def cos_table(F):
    """the kernel's table: the float64 values rounded once"""
    return cos_table64(F).astype(np.float32)


@lru_cache(maxsize=None)
def _matrices(F, n, hard=False, end_sign=True):
    """(Cf [n, F+1], Ci [F+1, n], mw [n]): c = Cf A, V = Ci c, with the lifter and its factors m_q folded into Ci"""
    t = cos_table64(F)
    q, k = np.arange(n)[:, None], np.arange(F + 1)[None, :]
    C = t[(q * k) % (2 * F)]
    if not end_sign:
        C = C.copy()
        C[:, F] = 1.0
    omega = np.full(F + 1, 2.0)
    omega[0] = omega[F] = 1.0
    w = np.ones(n) if hard else 0.5 * (1.0 + np.cos(PI * np.arange(n) / n))
    mw = w * np.where(np.arange(n) == 0, 1.0, 2.0)
    Cf = C * omega / (2.0 * F)
    Ci = (t[(q * k) % (2 * F)] * mw[:, None]).T
    return Cf, np.ascontiguousarray(Ci), mw


@lru_cache(maxsize=None)
def smoothing_norm(F, n):
    """||S||inf: the largest absolute row sum of S = Ci Cf"""
    Cf, Ci, _ = _matrices(F, n)
    return float(np.abs(Ci @ Cf).sum(1).max())


def power32(Y):
    F = Y.shape[-1] // 2
    re, im = Y[..., :F].astype(np.float32), Y[..., F:].astype(np.float32)
    with np.errstate(all="ignore"):
        return (re * re) + (im * im)                         # float32: each operation rounds once


def rho_of(ratio):
    """(rho float32, unit): the clamp, and NaN or 1 -> the frame is copied"""
    r = np.asarray(ratio, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        rho = np.minimum(np.maximum(np.where(np.isnan(r), np.float32(1), r), np.float32(0.25)), np.float32(4))
    return rho.astype(np.float32), np.isnan(r) | (rho == 1)


class Result:
    pass


def spec(Y, ratio, order, iterations, depth=DEPTH, max_gain=MAX_GAIN, fault=None, bound=True):
    """Y float32 [B, T, 2F], ratio float32 [1 or B, T] -> Result with out (float64 [B, T, 2F]; copied frames hold Y),
    env (float64 [B, T, F + 1]), copied / dead (bool [B, T]: copied bit for bit / without a usable Pmax), and, with `bound`,
    bound (float64 [B, T, 2F], per element) and env_bound (float64 [B, T])."""
    Y = np.asarray(Y, dtype=np.float32)
    B, T, F = Y.shape[0], Y.shape[1], Y.shape[2] // 2
    n, I = int(order), int(iterations)
    if fault == "no_iteration":
        I = 1
    ratio = np.broadcast_to(np.asarray(ratio, dtype=np.float32).reshape(-1, T), (B, T))
    rho, unit = rho_of(ratio)
    if fault == "unit_ratio_recomputed":                     # the branch that copies is gone: the NaN rule went with it
        unit = np.zeros_like(unit)
        with np.errstate(invalid="ignore"):
            rho = np.where(np.isnan(ratio), np.float32(0.25), rho).astype(np.float32)
    P = power32(Y)
    Pmax = P.max(-1)                                          # propagates NaN
    with np.errstate(invalid="ignore"):
        ok = (Pmax > 0) & (Pmax < np.inf)
    res = Result()
    res.out = Y.astype(np.float64)
    res.env = np.zeros((B, T, F + 1))
    res.dead, res.copied = ~ok, ~ok | unit
    res.bound = np.zeros((B, T, 2 * F))
    res.env_bound = np.zeros((B, T))
    if not ok.any():
        return res
    P64 = np.where(ok[..., None], P, 1.0).astype(np.float64)
    Pm = np.where(ok, Pmax, 1.0).astype(np.float64)
    with np.errstate(divide="ignore"):
        lnP = 0.5 * np.log(P64)
    floor = 0.5 * np.log(Pm) - depth
    L = lnP if fault == "no_floor" else np.maximum(lnP, floor[..., None])
    if fault == "no_floor":
        L = np.maximum(L, -1e4)                              # -inf would make every later figure NaN
    dc = np.minimum(floor, L[..., 0])[..., None] if fault == "dc_not_from_bin_1" else L[..., :1]
    Lx = np.concatenate([dc, L], -1)
    Cf, Ci, mw = _matrices(F, n, fault == "hard_lifter", fault != "end_sign_dropped")
    W = float(mw.sum())
    if bound:
        norm = smoothing_norm(F, n)
        Df = -(-(F + 1) // 64) + 6
        e_L = (2 * ULP_LOG + 1) * U * np.maximum(np.maximum(np.abs(Lx).max(-1), np.abs(0.5 * np.log(Pm))), np.abs(floor))
        E_A = e_L.copy()
    A, V_prev, E_V = Lx, Lx, None
    for _ in range(I):
        c = A @ Cf.T
        V = c @ Ci.T
        if bound:
            Amax = np.abs(A).max(-1) + E_A
            g_f = gamma(Df + 3) * Amax
            d_sum = (np.abs(c) * mw).sum(-1) + W * (E_A + g_f)
            E_V = norm * E_A + W * g_f + gamma(n + 1) * d_sum
            E_A = np.maximum(e_L, E_V)
        A = np.maximum(V_prev if fault == "max_against_v" else Lx, V)
        V_prev = V
    res.env = np.where(ok[..., None], V, 0.0)
    k = np.arange(1, F + 1, dtype=np.float32)
    with np.errstate(all="ignore"):
        x = (np.float32(1) / rho)[..., None] * k if fault == "gain_at_k_over_rho" else rho[..., None] * k      # float32 products
    x = x.astype(np.float32)
    if fault != "no_clamp_at_F":
        x = np.minimum(x, np.float32(F))
    i = np.minimum(np.floor(x).astype(np.int64), F - 1)
    f = x.astype(np.float64) - i
    Vi, Vi1 = np.take_along_axis(V, i, -1), np.take_along_axis(V, i + 1, -1)
    Vx = (1.0 - f) * Vi + f * Vi1
    d = Vx - V[..., 1:]
    dc_ = d if fault == "no_gain_clamp" else np.clip(d, -max_gain, max_gain)
    with np.errstate(over="ignore"):
        g = np.exp(dc_)
    gain = np.where((ok & ~unit)[..., None], g, 1.0)
    shifted = np.concatenate([gain, gain], -1) * Y.astype(np.float64)
    res.out = np.where(res.copied[..., None], Y.astype(np.float64), shifted)
    res.gain = gain
    if bound:
        E_V = np.where(ok, E_V, 0.0)
        E_Vx = E_V + gamma(3) * (np.abs(V).max(-1) + E_V)
        E_g = (E_Vx + E_V)[..., None] + U * (np.abs(d) + (E_Vx + E_V)[..., None])
        E_g = E_g * (1.0 + 4 * U) + 4 * U * U
        rel = np.expm1(E_g) + (2 * ULP_EXP + 1) * U
        with np.errstate(over="ignore", invalid="ignore"):
            res.bound = np.abs(Y.astype(np.float64)) * np.concatenate([gain * rel, gain * rel], -1)
        res.bound = np.where(res.copied[..., None], 0.0, res.bound)
        res.env_bound = E_V
    return res


# ------------------------------------------------------------------------------------- the float32 model, in the kernel's order
def _fma32(a, b, c):
    """fl32(a b + c): the product of two float32 is exact in float64, the sum rounds to double and then to float32 (a double
    rounding differs from the fused result in rare ties; the model is held to the bound, not to bits)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def model32(Y, ratio, order, iterations, depth=DEPTH, max_gain=MAX_GAIN):
    """(out float32 [B, T, 2F], env float32 [B, T, F + 1]) as the kernel forms them: float32 logarithms and exponentials (numpy's
    float32 routines stand in for the device's), the coefficient sums as 64 strided fma chains and a butterfly, V_k as one fma
    chain over q, the table rounded to float32"""
    Y = np.asarray(Y, dtype=np.float32)
    B, T, F = Y.shape[0], Y.shape[1], Y.shape[2] // 2
    n, n2 = int(order), 2 * F
    ratio = np.broadcast_to(np.asarray(ratio, dtype=np.float32).reshape(-1, T), (B, T)).reshape(-1)
    rho, unit = rho_of(ratio)
    Yf = Y.reshape(B * T, n2)
    P = power32(Yf)
    Pmax = P.max(-1)
    with np.errstate(invalid="ignore"):
        ok = (Pmax > 0) & (Pmax < np.inf)
    out, env = Yf.copy(), np.zeros((B * T, F + 1), np.float32)
    rows = np.nonzero(ok)[0]
    if not len(rows):
        return out.reshape(B, T, n2), env.reshape(B, T, F + 1)
    table = cos_table(F)
    P, N = P[rows], len(rows)
    with np.errstate(divide="ignore"):
        floor = np.float32(0.5) * np.log(Pmax[rows]).astype(np.float32) - np.float32(depth)
        L = np.maximum(np.float32(0.5) * np.log(P).astype(np.float32), floor[:, None]).astype(np.float32)
    Lx = np.concatenate([L[:, :1], L], -1)
    q = np.arange(n)
    sW = (np.where(q == 0, 1.0, 2.0) * (0.5 + 0.5 * np.cos(PI * q / n)) / n2).astype(np.float32)
    steps = -(-(F + 1) // 64)
    kpad = steps * 64
    omega = np.zeros(kpad, np.float32)
    omega[:F + 1] = 2.0
    omega[0] = omega[F] = 1.0
    kk = np.arange(kpad)
    Cq = table[(q[:, None] * kk[None, :]) % n2].reshape(n, steps, 64)                  # [n, steps, 64]
    Ck = table[(q[:, None] * np.arange(F + 1)[None, :]) % n2]                         # [n, F + 1]
    A = Lx
    for it in range(int(iterations)):
        a = np.zeros((N, kpad), np.float32)
        a[:, :F + 1] = A
        a = (a * omega).reshape(N, steps, 64)
        acc = np.zeros((N, n, 64), np.float32)
        for s in range(steps):
            acc = _fma32(a[:, None, s, :], Cq[None, :, s, :], acc)
        lanes = np.arange(64)
        for s in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[..., lanes ^ s]
        d = acc[..., 0] * sW                                                            # [N, n]
        V = np.zeros((N, F + 1), np.float32)
        for j in range(n):
            V = _fma32(d[:, j:j + 1], Ck[None, j, :], V)
        A = np.maximum(Lx, V)
    env[rows] = V
    k = np.arange(1, F + 1, dtype=np.float32)
    x = np.minimum(rho[rows][:, None] * k, np.float32(F)).astype(np.float32)
    i = np.minimum(x.astype(np.int64), F - 1)
    f = (x - i.astype(np.float32)).astype(np.float32)
    Vi, Vi1 = np.take_along_axis(V, i, -1), np.take_along_axis(V, i + 1, -1)
    vx = _fma32(f, Vi1, (np.float32(1) - f) * Vi)
    dd = np.clip(vx - V[:, 1:], np.float32(-max_gain), np.float32(max_gain)).astype(np.float32)
    g = np.exp(dd).astype(np.float32)
    moved = np.concatenate([g, g], -1) * Yf[rows]
    live = ~unit[rows]
    out[rows[live]] = moved[live]
    return out.reshape(B, T, n2), env.reshape(B, T, F + 1)


# ------------------------------------------------------------------------------------------------- the kernel cases and their data
KERNEL_F = (2, 5, 64, 130, 1024)
KERNEL_T = (1, 3, 17)
KERNEL_B = (1, 3)
KERNEL_ITERATIONS = (1, 3, 16)
FRAME_KINDS = ("comb", "random", "silent", "loud_bin", "equal", "nan", "inf", "range_200db")
RATIO_KINDS = ("ones", "up", "down", "per_frame", "special")
SPECIAL_RATIOS = (0.0, -1.0, 1e9, float("nan"), float("inf"), float("-inf"))


def orders(F):
    return sorted({2, min(F, 7), min(F, 64), min(F, 256)})


def make_frame(kind, F, g):
    """complex [F]; every frame's Pmax is a normal float32 or the frame is one the copy rule takes"""
    phase = np.exp(2j * PI * g.random(F))
    k = np.arange(1, F + 1)
    if kind == "comb":                                       # a harmonic comb under a two-formant envelope
        period = max(2.0, F / 9.0)
        teeth = 0.02 + np.maximum(0.0, np.cos(2 * PI * k / period)) ** 8
        envl = 1.0 / np.sqrt(1 + ((k - 0.2 * F) / (0.05 * F + 1)) ** 2) + 0.3 / np.sqrt(1 + ((k - 0.6 * F) / (0.1 * F + 1)) ** 2)
        return 3.0 * teeth * envl * phase
    if kind == "random":
        return (g.standard_normal(F) + 1j * g.standard_normal(F)) * 10.0 ** g.uniform(-2, 2)
    if kind == "silent":
        return np.zeros(F, complex)
    if kind == "loud_bin":
        X = np.zeros(F, complex)
        X[int(g.integers(F))] = 7.0 * phase[0]
        return X
    if kind == "equal":                                      # equal powers bit for bit: one float32 pair in every bin
        return np.full(F, np.float32(0.75) + 1j * np.float32(-1.25))
    if kind == "nan":
        X = (g.standard_normal(F) + 1j * g.standard_normal(F))
        X[int(g.integers(F))] = complex(float("nan"), 1.0)
        return X
    if kind == "inf":
        X = (g.standard_normal(F) + 1j * g.standard_normal(F))
        X[int(g.integers(F))] = complex(1.0, float("-inf"))
        return X
    if kind == "range_200db":                                # magnitudes from 1e-7 to 1e3: most of them under the floor
        return 10.0 ** np.linspace(-7.0, 3.0, F)[g.permutation(F)] * phase
    raise ValueError(kind)


def ratio_row(kind, T, g):
    if kind == "ones":
        return np.ones(T, np.float32)
    if kind == "up":
        return np.full(T, 2.0 ** (5 / 12), np.float32)
    if kind == "down":
        return np.full(T, 2.0 ** (-7 / 12), np.float32)
    if kind == "per_frame":
        return (2.0 ** g.uniform(-2.2, 2.2, T)).astype(np.float32)          # some leave [1/4, 4]
    first = int(g.integers(len(SPECIAL_RATIOS)))
    return np.array([SPECIAL_RATIOS[(first + t) % len(SPECIAL_RATIOS)] for t in range(T)], np.float32)


class Case:
    pass


def make_case(B, T, F, order, iterations, ratio_batch, seed=0, frame_offset=None):
    g = np.random.default_rng([B, T, F, order, iterations, ratio_batch, seed])
    c = Case()
    c.B, c.T, c.F, c.order, c.iterations, c.ratio_batch = B, T, F, order, iterations, ratio_batch
    c.depth, c.max_gain = np.float32(DEPTH), np.float32(MAX_GAIN)
    off = int(g.integers(len(FRAME_KINDS))) if frame_offset is None else frame_offset
    c.frame_kinds = [[FRAME_KINDS[(off + b * T + t) % len(FRAME_KINDS)] for t in range(T)] for b in range(B)]
    X = np.stack([np.stack([make_frame(c.frame_kinds[b][t], F, g) for t in range(T)]) for b in range(B)])
    with np.errstate(invalid="ignore"):
        c.Y = np.concatenate([X.real, X.imag], -1).astype(np.float32)
    roff = int(g.integers(len(RATIO_KINDS)))
    c.ratio_kinds = [RATIO_KINDS[(roff + r) % len(RATIO_KINDS)] for r in range(ratio_batch)]
    c.ratio = np.stack([ratio_row(kind, T, g) for kind in c.ratio_kinds])
    c.table = cos_table(F)
    c.name = f"B={B} T={T} F={F} order={order} iterations={iterations} ratio_batch={ratio_batch}"
    c._spec = None
    return c


def case_spec(case):
    if case._spec is None:
        case._spec = spec(case.Y, case.ratio, case.order, case.iterations, float(case.depth), float(case.max_gain))
    return case._spec


def kernel_cases(F):
    """every order of `orders(F)` with every T; iterations, B and the ratio form rotate so that each F meets every value of
    each, and each (T, order) pair meets both ratio forms at B = 3"""
    cases, n = [], 0
    for T in KERNEL_T:
        for order in orders(F):
            iterations = KERNEL_ITERATIONS[n % 3]
            for B, ratio_batch in (((1, 1), (3, 3)) if n % 2 == 0 else ((3, 1), (3, 3))):
                cases.append(make_case(B, T, F, order, iterations, ratio_batch, seed=n, frame_offset=n % len(FRAME_KINDS)))
            n += 1
    return cases


def flagship_case():
    """F at the cap with the largest order: two bins per lane everywhere"""
    return make_case(1, 8, 2048, 256, 3, 1, seed=99, frame_offset=0)


def compare(got_out, got_env, case, what=None):
    """the worst error / bound over the output's elements and the envelope rows; copied frames bit for bit; AssertionError
    beyond 1"""
    s, what = case_spec(case), what or case.name
    got_out = np.asarray(got_out, dtype=np.float32).reshape(case.Y.shape)
    same = bits(got_out) == bits(case.Y)
    assert same[s.copied].all(), f"{what}: a frame that the rule copies is not the input's bits"
    worst = 0.0
    live = ~s.copied
    if live.any():
        want, bound = s.out[live], s.bound[live]
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(got_out[live].astype(np.float64) - want)
        fin = np.isfinite(want) & (np.abs(want) < 3.0e38) & np.isfinite(bound)
        assert np.isfinite(got_out[live][fin]).all(), f"{what}: a value that is not finite where the spec's is"
        exact = fin & (bound == 0)
        assert (err[exact] == 0).all(), f"{what}: a zero of the input is not a zero of the output"
        part = fin & (bound > 0)
        if part.any():
            worst = float((err[part] / bound[part]).max())
    if got_env is not None:
        got_env = np.asarray(got_env, dtype=np.float32).reshape(s.env.shape)
        assert (bits(got_env[s.dead]) == 0).all(), f"{what}: the envelope row of a frame without a usable Pmax is not +0.0"
        alive = ~s.dead
        if alive.any():
            err = np.abs(got_env[alive].astype(np.float64) - s.env[alive]).max(-1)
            assert np.isfinite(err).all(), f"{what}: an envelope value that is not finite"
            worst = max(worst, float((err / s.env_bound[alive]).max()))
    assert worst <= 1.0, f"{what}: error / bound = {worst:.3f}"
    return worst


# ------------------------------------------------------------------------------------------------------------- the experiment
FORMANTS = ((600.0, 120.0, 0.0), (1400.0, 180.0, -6.0), (2900.0, 250.0, -12.0), (5200.0, 500.0, -25.0))     # fc, bw (Hz), gain (dB)


def formant_envelope(f):
    f = np.asarray(f, dtype=np.float64)
    s = sum(10.0 ** (gdb / 20.0) / np.sqrt(1.0 + ((f - fc) / bw) ** 2) for fc, bw, gdb in FORMANTS)
    return s / (1.0 + (f / 6000.0) ** 2) + 1e-3


def formant_tone(L, f0, fs=16000.0, seed=3):
    """all harmonics of f0 below 0.98 Nyquist under the envelope, fixed random phases"""
    h = np.arange(1, int(0.98 * fs / 2 / f0) + 1)
    ph = np.random.default_rng(seed).uniform(0, 2 * PI, len(h))
    n = np.arange(L)
    x = np.zeros(L)
    for hh, p in zip(h, ph):
        x += formant_envelope(hh * f0) * np.cos(2 * PI * hh * f0 * n / fs + p)
    return x


def order_for(fs, f0, factor=0.5):
    return int(min(max(round(factor * fs / f0), 4), MAX_ORDER))


def counted_partials(f0, rho, fs=16000.0):
    """the harmonics h whose target rho h f0 lies below 0.95 Nyquist and within 50 dB of the envelope's maximum"""
    top = formant_envelope(np.linspace(0.0, fs / 2, 8001)).max()
    h = np.arange(1, int(0.98 * fs / 2 / f0) + 1)
    target = formant_envelope(rho * h * f0)
    return h[(rho * h * f0 < 0.95 * fs / 2) & (20 * np.log10(target / top) > -50.0)]


def db_errors(amplitudes, f0, rho, h):
    """(rms, largest) dB error of partial amplitudes against E(rho h f0)"""
    e = 20.0 * np.log10(np.asarray(amplitudes) / formant_envelope(rho * h * f0))
    return float(np.sqrt(np.mean(e ** 2))), float(np.abs(e).max())


def experiment(f0, semitones, F=128, fs=16000.0, iterations=16, hard=False, order_factor=0.5):
    """The single-frame idealisation: one periodic-Hann frame of the formant tone, its true envelope, the gain read at each
    partial's own frequency.  -> (corrected rms, plain rms, corrected max, plain max) in dB over `counted_partials`."""
    n_fft, rho = 2 * F, 2.0 ** (semitones / 12.0)
    x = formant_tone(n_fft, f0, fs)
    w = 0.5 - 0.5 * np.cos(2 * PI * np.arange(n_fft) / n_fft)
    X = np.fft.rfft(x * w)[1:]
    Y = np.concatenate([X.real, X.imag])[None, None].astype(np.float32)
    n = min(order_for(fs, f0, order_factor), F)
    V = spec(Y, np.ones((1, 1), np.float32), n, iterations, fault="hard_lifter" if hard else None, bound=False).env[0, 0]
    h = counted_partials(f0, rho, fs)
    kappa = h * f0 * n_fft / fs

    def at(pos):
        pos = np.minimum(pos, F)
        i = np.minimum(np.floor(pos).astype(int), F - 1)
        return (1 - (pos - i)) * V[i] + (pos - i) * V[i + 1]

    gain = np.exp(np.clip(at(rho * kappa) - at(kappa), -MAX_GAIN, MAX_GAIN))
    source = formant_envelope(h * f0)
    corrected, plain = db_errors(source * gain, f0, rho, h), db_errors(source, f0, rho, h)
    return corrected[0], plain[0], corrected[1], plain[1]


# ------------------------------------------------------------------------------------ the float64 pipeline of `transpose`
def projected_amplitudes(x, freqs, fs, lo, hi):
    """least-squares amplitudes of sinusoids at `freqs` (Hz) in x[lo:hi] under a Hann window"""
    n = np.arange(lo, hi)
    w = np.sqrt(0.5 - 0.5 * np.cos(2 * PI * (n - lo + 0.5) / (hi - lo)))
    cols = np.concatenate([np.cos(2 * PI * np.outer(n, freqs) / fs), np.sin(2 * PI * np.outer(n, freqs) / fs)], 1)
    sol = np.linalg.lstsq(cols * w[:, None], x[lo:hi] * w, rcond=None)[0]
    return np.hypot(sol[:len(freqs)], sol[len(freqs):])


def partial_error(z, f0, rho, fs=16000.0, lo=None, hi=None):
    """(rms, largest) dB error of z's partials at rho h f0 against E(rho h f0), by projection in the steady window
    [L / 4, 3 L / 4) unless given; every partial below Nyquist is fitted, the counted ones are scored"""
    L = len(z)
    lo, hi = L // 4 if lo is None else lo, 3 * L // 4 if hi is None else hi
    h_all = np.arange(1, int(0.98 * fs / 2 / f0) + 1)
    h_all = h_all[rho * h_all * f0 < 0.98 * fs / 2]
    amp = projected_amplitudes(np.asarray(z, dtype=np.float64), rho * h_all * f0, fs, lo, hi)
    h = counted_partials(f0, rho, fs)
    return db_errors(amp[np.isin(h_all, h)], f0, rho, h)


def transpose64(x, semitones, n_fft=256, hop=64, order=None, f0=440.0, fs=16000.0, preserve=True, iterations=16):
    """`transpose` in float64 numpy: the stretch specification's STFT, phase-locked re-timing (tests/stft_stretch_spec.py), this
    file's correction at rho = num / den on the re-timed frames (rounded to float32: P is a float32 quantity), the inverse, and
    a windowed-sinc read at den / num"""
    import stft_stretch_spec as R
    num, den = R.semitone_ratio(semitones)
    L = len(x)
    T, extra = -(-L // hop), n_fft // hop - 1
    X = R.stft(np.concatenate([x, np.zeros(T * hop - L)]), n_fft, hop, T + extra)
    T_out = max(1, int(round(T * num / den)))
    pos = np.concatenate([R.positions(T, n_out=T_out), np.arange(T, T + extra, dtype=np.float32)])[None]
    Y = R.stretch(R.pack(X), pos, hop).out[0]
    if preserve:
        order = order_for(fs, f0) if order is None else order
        Yp = np.concatenate([Y.real, Y.imag], -1)[None].astype(np.float32)
        out = spec(Yp, np.full((1, Yp.shape[1]), num / den, np.float32), order, iterations, bound=False).out[0]
        Y = out[:, :n_fft // 2] + 1j * out[:, n_fft // 2:]
    y = R.istft(Y, n_fft, hop, T_out * hop)
    return R.resample_bandlimited(y, num, den, L)
