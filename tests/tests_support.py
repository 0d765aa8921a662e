"""Helpers shared by CPU and GPU tests (test infrastructure)."""
import collections
import math

import numpy as np
import torch


def trajectory_case(golden_dir, tag):
    """(fixture, initial state dict, constructor kwargs, the two input batches) of tests/golden/train_trajectory.npz
    (generated from the imported reference by oracle/make_golden.py::train_trajectory_fixtures)."""
    z = np.load(golden_dir / "train_trajectory.npz")
    if tag == "small":
        sd = {k[len("small::w::"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("small::w::")}
        kw = dict(in_channel=2, num_hidden_channels=32, n_res_block=2, num_residual_channels=8, embed_dim=16,
                  num_embeddings=64)
        xs = [torch.from_numpy(z[f"small::x{i}"]) for i in range(2)]
        return z, sd, kw, xs
    zw = np.load(golden_dir / "vqvae_default_tiny.npz")
    sd = {k[3:]: torch.from_numpy(zw[k]) for k in zw.files if k.startswith("w::")}
    g = torch.Generator().manual_seed(int(z["full::x_seed"]))
    xs = [torch.randn(8, 2, 128, 512, generator=g) for _ in range(2)]
    for i, xb in enumerate(xs):
        xb[:, 1].tanh_()
        assert np.array_equal(xb.reshape(-1)[:64].numpy(), z[f"full::x{i}_head"]), "the seeded inputs must be the fixture's"
        assert abs(xb.double().sum().item() - float(z[f"full::x{i}_sum"])) < 1e-6 * xb.numel()
    return z, sd, dict(in_channel=2), xs


# ---------------------------------------------------------------------------------------------------------------------
# Float64 specification of the categorical draw (temperature, top-k, top-p, inverse-CDF draw): numpy alone, no GPU and none
# of the project's kernels.  tests/test_sampling_spec_host.py holds it to oracle/prior_oracle.py; tests/test_sampling_draw_gpu.py
# holds the draw kernel to it.  The generators below are shared by the two files: same rows, same seeds, same filters.
SAMPLING_TAU = 2.0 ** -17
SAMPLING_SHAPES = (1, 2, 63, 64, 65, 500, 512, 513, 1000, 1024)
SAMPLING_TEMPERATURES = (0.05, 0.7, 1.0, 10.0)
SAMPLING_TOP_K = (0, 1, 5, 40, "n", "n+7")
# (top_k, top_p): every top_k alone, every top_p alone, both together.  top_p: 0, "one" (keeps one class), "p80" (about 0.8),
# 1.0 and "tie" (the cut between two equal logits; only rows that carry such a tie resolve it)
SAMPLING_FILTERS = tuple((k, 0.0) for k in SAMPLING_TOP_K) + (
    (0, "one"), (0, "p80"), (0, 1.0), (0, "tie"), (5, "p80"), (5, 1.0), (40, "one"), (40, "p80"), (40, 1.0), ("n+7", "p80"))
SAMPLING_TOP_P_MARGIN = 1e-5
SamplingSpec = collections.namedtuple("SamplingSpec", "lg kept cdf prob")
SamplingCase = collections.namedtuple("SamplingCase", "name logits temperature top_k top_p stride")


def sampling_scaled_logits(logits, temperature):
    """float32(logits) * (float32(1) / float32(T)): one fp32 multiply by the fp32 reciprocal, the only fp32 step of the spec
    (IEEE: the same bits on every machine).  For the temperatures of SAMPLING_TEMPERATURES the reciprocal equals
    float32(1 / T) (checked in tests/test_sampling_spec_host.py)."""
    inv = np.float32(1.0) / np.float32(temperature)
    return (np.asarray(logits, dtype=np.float32) * inv).astype(np.float32)


def _top_k_kept(x, top_k):
    """x float64 [n] -> bool [n]: finite and not `< kth` (k clamped to n), as oracle/prior_oracle.py."""
    n = x.shape[0]
    kept = np.isfinite(x)
    k = min(int(top_k), n)
    if k > 0:
        kept &= ~(x < np.sort(x)[n - k])
    return kept


def _top_p_cumulatives(x, kept):
    """(order, cum): the STABLE descending order of the row (among equal logits the lower index first; removed classes
    last) and the float64 cumulative probabilities along it."""
    f = np.where(kept, x, -np.inf)
    order = np.argsort(-f, kind="stable")
    e = np.exp(f[order] - f[order[0]])
    cum = np.cumsum(e)
    return order, cum / cum[-1]


def sampling_top_p_cumulatives(logits, temperature, top_k):
    """The cumulative probabilities that DECIDE a top-p cut of this row after top-k: sorted position s is removed when
    cum[s - 1] > top_p, so the last kept class's own cumulative (1.0) decides nothing and is left out."""
    x = sampling_scaled_logits(logits, temperature).astype(np.float64)
    kept = _top_k_kept(x, top_k)
    _, cum = _top_p_cumulatives(x, kept)
    return cum[:max(int(kept.sum()) - 1, 0)]


def sampling_spec(logits, temperature, top_k, top_p):
    """Float64 specification of one row of the draw kernel.  logits float32 [n]; returns SamplingSpec(lg, kept, cdf, prob):
      1. lg = float32(logits) * float32(1 / T), one fp32 multiply; everything after it is float64 of lg;
      2. top-k as oracle/prior_oracle.py: k clamped to n, classes `< kth` removed (ties on the k-th value stay);
      3. top-p on a STABLE descending sort (among equal logits the lower index comes first: the kernel's documented tie
         rule, which torch.sort leaves open): sorted position s is removed when cum[s - 1] > float32(top_p);
      4. prob = softmax over the kept classes, cdf = its inclusive cumulative sum in class order, cdf[-1] == 1.
    A class the caller masked with -inf is not kept."""
    lg = sampling_scaled_logits(logits, temperature)
    x = lg.astype(np.float64)
    kept = _top_k_kept(x, top_k)
    if top_p > 0.0:
        order, cum = _top_p_cumulatives(x, kept)
        remove = np.zeros(x.shape[0], dtype=bool)
        remove[1:] = cum[:-1] > float(np.float32(top_p))
        kept = kept.copy()
        kept[order[remove]] = False
    prob = np.where(kept, np.exp(x - x[kept].max()), 0.0)
    prob = prob / prob.sum()
    cdf = np.cumsum(prob)
    return SamplingSpec(lg, kept, cdf / cdf[-1], prob)


def sampling_accepts(spec, u, drawn, tau=SAMPLING_TAU):
    """The one acceptance rule of every draw check, vectorised over u [R] (float32 values) and drawn [R]: class i is
    accepted for u when it is a KEPT class of NON-ZERO probability and its float64 interval [cdf[i-1], cdf[i]) meets
    [u (1 - tau), u (1 + tau)].  Returns (ok [R], first [R], last [R]): the accepted classes are the non-zero classes from
    `first` to `last`, found with searchsorted on the CDF of the non-zero classes (a class between the two whose interval
    is empty in float64 but not in exact arithmetic lies inside the window and is accepted).

    tau = 2^-17 is derived, not measured.  The kernel draws the first class with inc > u * total, inc an fp32 prefix sum of
    terms expf(lg - max).  (a) Each term carries at most about 20 eps of relative error, eps = 2^-24: the fp32 subtraction
    lg - max is off by half an ulp of a difference of up to 103 (below -103 expf is under fp32 resolution and the term is
    0), that is 103 * 2^-24 / 2 ~ 16 eps absolute in the exponent = 16 eps relative in exp, plus a few eps of expf itself.
    (b) Each term passes through at most 22 fp32 additions on its way into a prefix or the total: 6 levels of the 64-lane
    wave scan and up to 16 wave totals, one eps each.  (c) All terms are non-negative, so relative errors do not amplify:
    inc and total are each within about 20 + 22 = 42 eps of their exact values, the boundary inc / total within about 84,
    and the product u * total adds one more: about 90 eps, rounded up to 128 eps = 2^-17.

    An ADDITION to the derived tau, not part of it.  The relative bound does not reach below fp32 resolution, and at
    u = 0 the relative window is empty.  A term under the fp32 normal range, 2^-126 of the largest term (which is exactly
    1, so total >= 1), may be flushed to 0 or lose all its digits.  n such terms move a boundary by at most n 2^-126 (1.2e-35 at n = 1024), a property of the number format; the
    window is widened by that much on both sides, so at u = 0 a leading class of probability 1e-60 may be skipped."""
    u = np.asarray(u, dtype=np.float64)
    drawn = np.asarray(drawn, dtype=np.int64)
    nz = np.flatnonzero(spec.kept & (spec.prob > 0.0))
    cn = spec.cdf[nz]
    last_i = nz.shape[0] - 1
    tiny = spec.cdf.shape[0] * 2.0 ** -126
    a = np.minimum(np.searchsorted(cn, u * (1.0 - tau) - tiny, side="right"), last_i)   # first class with cdf > the lower end
    b = np.minimum(np.searchsorted(cn, u * (1.0 + tau) + tiny, side="right"), last_i)   # the class that holds the upper end
    pos = np.minimum(np.searchsorted(nz, drawn), last_i)
    ok = (nz[pos] == drawn) & (pos >= a) & (pos <= b)
    return ok, nz[a], nz[b]


def sampling_float64_draw(spec, u):
    """The float64 inverse-CDF draw itself: the first non-zero class whose cdf exceeds u."""
    nz = np.flatnonzero(spec.kept & (spec.prob > 0.0))
    return nz[np.minimum(np.searchsorted(spec.cdf[nz], np.asarray(u, dtype=np.float64), side="right"), nz.shape[0] - 1)]


def sampling_pick_top_p(logits, temperature, top_k, what):
    """A float32 top_p for this row, at the float32 midpoint between two adjacent deciding cumulatives (0 counts as one), or
    None where the row has no such value: "one" keeps one class, "p80" is the midpoint of the gap that holds 0.8 (or of the
    nearest gap wide enough), "tie" cuts between the second and third of three equal logits, 1.0 is 1.0 itself and is
    used only where the last deciding cumulative lies SAMPLING_TOP_P_MARGIN below it.  0.0 stays 0.0."""
    if what == 0.0:
        return 0.0
    cum = sampling_top_p_cumulatives(logits, temperature, top_k)
    if what == 1.0:
        return 1.0 if (cum.shape[0] == 0 or cum[-1] <= 1.0 - 4 * SAMPLING_TOP_P_MARGIN) else None
    edges = np.concatenate([[0.0], cum, [1.0]])
    wide = np.flatnonzero(np.diff(edges) >= 4 * SAMPLING_TOP_P_MARGIN)
    if what == "one":
        j = 0 if 0 in wide else None
    elif what == "p80":
        j0 = int(np.searchsorted(edges, 0.8, side="right")) - 1
        j = int(wide[np.argmin(np.abs(wide - j0))]) if wide.shape[0] else None
    else:
        assert what == "tie", what
        x = sampling_scaled_logits(logits, temperature).astype(np.float64)
        kept = _top_k_kept(x, top_k)
        order, _ = _top_p_cumulatives(x, kept)
        sv = x[order][:int(kept.sum())]
        trip = np.flatnonzero((sv[:-2] == sv[1:-1]) & (sv[1:-1] == sv[2:])) if sv.shape[0] >= 3 else np.zeros(0, dtype=int)
        trip = [int(s) for s in trip if s + 1 in wide]      # edges[s + 1] = cum[s], edges[s + 2] = cum[s + 1]
        j = trip[0] + 1 if trip else None
    if j is None:
        return None
    return float(np.float32(0.5 * (edges[j] + edges[j + 1])))


def sampling_rows(n):
    """The rows of one shape: [(name, float32 logits [n], temperature)], seeded by n alone."""
    g = np.random.default_rng(7000 + n)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    rows = [("randn1", f32(g.standard_normal(n)), 1.0), ("randn1_T0.05", f32(g.standard_normal(n)), 0.05)]
    r3 = f32(3.0 * g.standard_normal(n))
    rows += [(f"randn3_T{t}", r3, t) for t in SAMPLING_TEMPERATURES]
    rows.append(("randn10", f32(10.0 * g.standard_normal(n)), 0.7))
    r = f32(g.standard_normal(n))
    r[n // 3] += 60.0
    rows.append(("dominant", r, 1.0))
    rows.append(("near+80", f32(g.standard_normal(n)) + np.float32(80.0), 0.7))
    rows.append(("near-80", f32(g.standard_normal(n)) - np.float32(80.0), 10.0))
    r = f32(3.0 * g.standard_normal(n))
    r[1::3] = -np.inf                                    # a third of the classes masked by the caller
    rows.append(("masked", r, 1.0))
    r = f32(3.0 * g.standard_normal(n))                  # exact ties on the k-th value, k = 5 and 40
    for k in (5, 40):
        if n >= k + 4:
            order = np.argsort(-r, kind="stable")
            r[order[[k + 1, n // 2, n - 1]]] = r[order[k - 1]]
    rows += [("ties_k", r, 1.0), ("ties_k_T0.7", r, 0.7)]
    r = f32(3.0 * g.standard_normal(n))                  # three equal logits where the cumulative probability passes 0.8
    if n >= 8:
        order = np.argsort(-r, kind="stable")
        _, cum = _top_p_cumulatives(r.astype(np.float64), np.ones(n, dtype=bool))
        s = min(int(np.searchsorted(cum, 0.8)), n - 3)
        r[order[s:s + 3]] = r[order[s + 1]]
    rows.append(("ties_p", r, 1.0))
    return rows


def sampling_cases(n):
    """Every (row, filter) case of one shape.  Every second case has a row stride larger than n (the GPU tests put NaN
    behind the row).  A top_p the row cannot resolve (see sampling_pick_top_p) leaves that case out."""
    cases = []
    for name, logits, t in sampling_rows(n):
        for k, p in SAMPLING_FILTERS:
            top_k = n if k == "n" else n + 7 if k == "n+7" else k
            top_p = sampling_pick_top_p(logits, t, top_k, p)
            if top_p is None:
                continue
            cases.append(SamplingCase(f"{name}/k{k}/p{p}", logits, t, top_k, top_p, n + (5 if len(cases) % 2 else 0)))
    return cases


def sampling_sweep_uniforms(spec, others=16, ulps=128):
    """The boundary sweep of one case: (u float32 [B * (2 ulps + 1)], boundary index [same] into the non-zero classes).
    Boundaries: every CDF boundary next to a zero-probability class (one lies between the two non-zero classes it parts, or
    before the first), plus `others` of the rest, evenly spread.  Around u0 = float32(boundary), every float32 within
    `ulps` ulps of it, inside [0, 1)."""
    nz = np.flatnonzero(spec.kept & (spec.prob > 0.0))
    m = nz.shape[0]
    if m < 2:
        return np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64)
    gap = np.diff(nz) > 1                                # a zero-probability class between non-zero classes j and j + 1
    # (with zero-probability classes before the first non-zero one, that boundary is u = 0: the end checks draw it)
    near_zero = np.flatnonzero(gap)
    rest = np.flatnonzero(~gap)
    if rest.shape[0] > others:
        rest = rest[np.linspace(0, rest.shape[0] - 1, others).astype(np.int64)]
    bidx = np.sort(np.concatenate([near_zero, rest]))
    u0 = spec.cdf[nz[bidx]].astype(np.float32)
    bits = u0.view(np.int32).astype(np.int64)[:, None] + np.arange(-ulps, ulps + 1, dtype=np.int64)[None, :]
    ok = (bits >= 0) & (bits < int(np.float32(1.0).view(np.int32)))
    u = bits.clip(0, int(np.float32(1.0).view(np.int32)) - 1).astype(np.int32).view(np.float32)
    b = np.broadcast_to(bidx[:, None], u.shape)
    return np.ascontiguousarray(u[ok]), np.ascontiguousarray(b[ok])


def sampling_grid_rows():
    """The rows of the stratified grid u = (j + 0.5) / 2^18: (name, logits, temperature, top_k, top_p)."""
    g = np.random.default_rng(7999)
    r512 = np.asarray(g.standard_normal(512), dtype=np.float32)
    r513 = np.asarray(3.0 * g.standard_normal(513), dtype=np.float32)
    m513 = r513.copy()
    m513[512] = -np.inf                                  # the mask token, excluded by the caller
    return [("n512", r512, 1.0, 0, 0.0), ("n513", r513, 0.7, 0, 0.0), ("n513_masked_k40", m513, 1.0, 40, 0.0)]


def sampling_grid_uniforms():
    return ((np.arange(2 ** 18, dtype=np.float64) + 0.5) / 2.0 ** 18).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# Float64 specifications of the prior's row-wise kernels (LayerNorm forward and backward with the fused residual and
# dropout, the label-smoothing criterion, the few-rows linear layer): closed forms in torch float64 on the CPU, no autograd
# and none of the project's kernels.  tests/test_prior_row_ops_host.py holds them to float64 autograd and shows what
# `compare_rows` accepts and rejects; tests/test_prior_row_ops_gpu.py holds the kernels to them.
ROW_OPS_MARGIN = 8.0           # a kernel may be this many times as far from the float64 spec as float32 torch is
ROW_OPS_FLOOR = 2.0 ** -23     # ... or as one float32 ulp, where float32 torch happens to be exact
RowCheck = collections.namedtuple("RowCheck", "what err yardstick ratio")


def _f64(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def _ln_stats(x, res, eps, keep, p):
    """z = drop(x) + res, its row mean, 1 / sqrt(biased variance + eps) and xhat, all float64."""
    z = _f64(x)
    if keep is not None:
        z = z * _f64(keep) / (1.0 - p)
    if res is not None:
        z = z + _f64(res)
    mean = z.mean(dim=-1, keepdim=True)
    var = (z - mean).pow(2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return rstd, (z - mean) * rstd


def layernorm_spec(x, res, gamma, beta, eps, keep=None, p=0.0):
    """y = LayerNorm(drop(x) + res) * gamma + beta over the last dimension; drop = x * keep / (1 - p) for a boolean keep
    mask (None: no dropout)."""
    _, xhat = _ln_stats(x, res, eps, keep, p)
    return xhat * _f64(gamma) + _f64(beta)


def layernorm_bwd_spec(x, res, gamma, dy, eps, keep=None, p=0.0):
    """(dz, dx, dgamma, dbeta) of layernorm_spec for the upstream gradient dy [M, D], by the formulas in the header of
    layernorm_bwd_kernel: g = dy * gamma, dz = rstd * (g - mean(g) - xhat * mean(g * xhat)) is the gradient of z (and of
    the residual), dx = dz * keep / (1 - p) that of x (dz itself without dropout), dgamma = sum over rows of dy * xhat,
    dbeta = sum over rows of dy."""
    rstd, xhat = _ln_stats(x, res, eps, keep, p)
    dy = _f64(dy)
    g = dy * _f64(gamma)
    dz = rstd * (g - g.mean(dim=-1, keepdim=True) - xhat * (g * xhat).mean(dim=-1, keepdim=True))
    dx = dz if keep is None else dz * _f64(keep) / (1.0 - p)
    return dz, dx, (dy * xhat).sum(dim=0), dy.sum(dim=0)


def label_smoothing_spec(logits, target, num_classes, smoothing, grad_scale):
    """(row_loss [M], dlogits [M, K]) of the reference's LabelSmoothingLoss (oracle/prior_oracle.py::label_smoothing_loss):
    true_dist = smoothing / (num_classes - 1) in every one of the K columns and 1 - smoothing at the target;
    row_loss = -sum_k true_dist[k] * log_softmax(logits)[k]; dlogits = d(sum of row_loss)/d(logits) * grad_scale
    = (softmax * sum_k true_dist[k] - true_dist) * grad_scale.  For K == num_classes true_dist sums to 1 and this is
    (softmax - true_dist) * grad_scale; for K != num_classes (a mask token among the logits) it does not, and
    (softmax - true_dist) is not the gradient of the loss (tests/test_prior_row_ops_host.py holds this form to autograd)."""
    lg = _f64(logits)
    v = lg - lg.max(dim=1, keepdim=True).values
    logp = v - torch.log(torch.exp(v).sum(dim=1, keepdim=True))
    true = torch.full_like(logp, smoothing / (num_classes - 1))
    true[torch.arange(lg.shape[0]), torch.as_tensor(target).cpu().long()] = 1.0 - smoothing
    return -(true * logp).sum(dim=1), (torch.exp(logp) * true.sum(dim=1, keepdim=True) - true) * grad_scale


def linear_rows_spec(x, W, bias, res, relu):
    """[relu](x W^T + bias + res) with the torch weight layout W [N, K]."""
    y = _f64(x) @ _f64(W).t()
    if bias is not None:
        y = y + _f64(bias)
    if res is not None:
        y = y + _f64(res)
    return y.clamp(min=0.0) if relu else y


def row_error(got, ref):
    """The metric of compare_rows.  A tensor with rows (two or more dimensions; rows = the last dimension): the largest
    over rows of max|err_row| / max|ref_row|, the scale clamped from below at 2^-100 (an all-zero reference row).  A
    vector: max|err| / max|ref|.  A non-finite value anywhere in `got` gives inf."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} against {tuple(ref.shape)}"
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    if ref.dim() >= 2:
        scale = ref.abs().amax(dim=-1).clamp(min=2.0 ** -100)
        return float((err.amax(dim=-1) / scale).max())
    return float(err.max() / ref.abs().max().clamp(min=2.0 ** -100))


def compare_rows(got, ref, yardstick, what, margin=ROW_OPS_MARGIN):
    """Holds `got` (a kernel's output) to the float64 reference `ref`, with the error of `yardstick` -- a float32 torch
    evaluation of the same operation on the same data -- as the measure of what float32 can do there:
        row_error(got, ref) <= margin * max(row_error(yardstick, ref), 2^-23).
    Both round O(log D) to O(D) times in different orders, hence the margin of 8; a poorly conditioned (cancelling) sum
    raises the yardstick's error with the kernel's, so the conditioning is priced in, not guessed.  Returns the RowCheck
    (what, err, yardstick, ratio) for the record; raises AssertionError past the bound."""
    err = row_error(got, ref)
    yard = max(row_error(yardstick, ref), ROW_OPS_FLOOR)
    assert math.isfinite(yard), f"{what}: the float32 yardstick itself is not finite"
    ratio = err / yard
    assert ratio <= margin, f"{what}: error {err:.3e} is {ratio:.1f} times the float32 yardstick {yard:.3e} (margin {margin:g})"
    return RowCheck(what, err, yard, ratio)


# float32 torch evaluations of the same operations, written with plain tensor operations on the CPU: the yardsticks of the
# GPU tests, and what the host tests apply their mutants to
def layernorm_f32(x, res, gamma, beta, eps, keep=None, p=0.0, mean_count=None, one_pass=False):
    """(y, rstd, xhat) in float32.  The two switches are the host tests' mutants: `mean_count` divides the row sums by
    this count, not by D; `one_pass` takes the variance as E[z^2] - mean^2."""
    z = x.float()
    D = z.shape[-1]
    if keep is not None:
        z = z * keep.float() / (1.0 - p)
    if res is not None:
        z = z + res.float()
    mean = z.sum(dim=-1, keepdim=True) / float(mean_count or D)
    if one_pass:
        var = (z * z).sum(dim=-1, keepdim=True) / float(D) - mean * mean
    else:
        var = (z - mean).pow(2).sum(dim=-1, keepdim=True) / float(D)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * rstd
    return xhat * gamma.float() + beta.float(), rstd, xhat


def layernorm_bwd_f32(x, res, gamma, dy, eps, keep=None, p=0.0):
    _, rstd, xhat = layernorm_f32(x, res, gamma, torch.zeros_like(gamma), eps, keep, p)
    dy = dy.float()
    g = dy * gamma.float()
    dz = rstd * (g - g.mean(dim=-1, keepdim=True) - xhat * (g * xhat).mean(dim=-1, keepdim=True))
    dx = dz if keep is None else dz * keep.float() / (1.0 - p)
    return dz, dx, (dy * xhat).sum(dim=0), dy.sum(dim=0)


def label_smoothing_f32(logits, target, num_classes, smoothing, grad_scale, off=None, unit_sum=False):
    """The host tests' mutants: `off`, another value for the off-target entries of true_dist; `unit_sum`, the gradient
    (softmax - true_dist) whatever true_dist sums to."""
    logp = logits.float().log_softmax(dim=1)
    true = torch.full_like(logp, smoothing / (num_classes - 1) if off is None else off)
    true[torch.arange(logp.shape[0]), target.long()] = 1.0 - smoothing
    return -(true * logp).sum(dim=1), (logp.exp() * (1.0 if unit_sum else true.sum(dim=1, keepdim=True)) - true) * grad_scale


def linear_rows_f32(x, W, bias, res, relu):
    y = x.float() @ W.float().t()
    if bias is not None:
        y = y + bias.float()
    if res is not None:
        y = y + res.float()
    return y.clamp(min=0.0) if relu else y


def layernorm_data(kind, M, D, gen):
    """x [M, D] float32: "randn"; "offset": rows of mean 100 and standard deviation 1, every third of standard deviation 1e-3
    (poorly conditioned: a one-pass variance fails here); "const": randn with the first and the last row constant
    (variance 0: rstd = 1 / sqrt(eps), y = beta)."""
    x = torch.randn(M, D, generator=gen)
    if kind == "offset":
        x[2::3] *= 1e-3
        x += 100.0
    elif kind == "const":
        x[0] = 3.75                                      # (few significant bits: a row's sum is exact in fp32 in any order)
        x[-1] = -0.25
    else:
        assert kind == "randn", kind
    return x
