"""Helpers shared by CPU and GPU tests (test infrastructure)."""
import collections
import functools
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
    ref = torch.as_tensor(ref).detach()
    if ref.is_cuda:                                       # (a reference kept on a device is compared there: 16 M outputs)
        got, ref = torch.as_tensor(got).detach().to(ref.device).double(), ref.double()
    else:
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


# ---------------------------------------------------------------------------------------------------------------------
# Float64 specifications of the small kernels of the VQ-VAE training step (csrc/train_ops.hip, and vq_finalize / embed_code
# of csrc/vq_nearest.hip), in the style of the row-ops block above: closed forms in torch float64 on the CPU, no autograd and
# none of the project's kernels; beside each a float32 torch evaluation of the same operation, the yardstick of
# `compare_rows`, whose keyword switches are the host tests' mutants.  tests/test_train_ops_host.py holds the specs to
# float64 autograd of the reference formulation and shows what the comparisons reject; tests/test_train_ops_gpu.py holds
# the kernels to them.  Operations that round nowhere (a selection, a gather) are held bit for bit: `same_bits`.
TRAIN_OPS_GRID_CAP = 8192 * 256        # threads of the largest grid-stride launch of csrc/train_ops.hip (`grid_for`)


def same_bits(got, want):
    """Bit for bit (NaN payloads and the sign of zero included) after `want` is cast to float32."""
    got, want = torch.as_tensor(got).detach().cpu(), torch.as_tensor(want).detach().cpu().float()
    return got.dtype == torch.float32 and got.shape == want.shape and bool(torch.equal(got.contiguous().view(torch.int32),
                                                                                     want.contiguous().view(torch.int32)))


def relu_bwd_spec(dy, y):
    """where(y > 0, dy, 0): a selection, as torch's threshold_backward -- a NaN or inf of dy where y <= 0 gives 0, and
    y = -0.0 masks like +0.0."""
    dy = _f64(dy)
    return torch.where(_f64(y) > 0, dy, torch.zeros_like(dy))


def relu_bwd_f32(dy, y, gate_ge=False, multiply=False):
    """Mutants: `gate_ge`, the gate as y >= 0; `multiply`, the gate as a factor (a masked NaN leaks through)."""
    dy, y = dy.float(), y.float()
    keep = (y >= 0) if gate_ge else (y > 0)
    return dy * keep.float() if multiply else torch.where(keep, dy, torch.zeros_like(dy))


def relu_inplace_spec(x):
    """x < 0 ? 0 : x -- NaN stays NaN, -0.0 stays -0.0."""
    x = _f64(x)
    return torch.where(x < 0, torch.zeros_like(x), x)


def axpy_spec(a, b, alpha):
    """a + alpha b, alpha the float32 value the C-ABI receives."""
    return _f64(a) + float(np.float32(alpha)) * _f64(b)


def axpy_f32(a, b, alpha):
    return a.float() + torch.tensor(alpha, dtype=torch.float32) * b.float()


def vq_bwd_spec(dq, z, q_st, g_diff):
    """Quantiser backward (bottleneck.py:94-95): dz = dq + 2 g_diff (z - q_st) / numel(z) -- the straight-through gradient
    plus that of diff = mean((q.detach() - z)^2), with the forward's q_st = z + (q - z) standing for q.  dq may be a
    row-strided view: the values are the same."""
    z = _f64(z)
    return _f64(dq).reshape(z.shape) + 2.0 * float(g_diff) * (z - _f64(q_st)) / z.numel()


def vq_bwd_f32(dq, z, q_st, g_diff, two=2.0):
    """Mutant: `two`, the coefficient's numerator (1: the gradient of half the commitment term)."""
    z = z.float()
    coef = torch.tensor(two * float(g_diff), dtype=torch.float32) / float(z.numel())
    return dq.float().reshape(z.shape) + coef * (z - q_st.float())


def add_gate_rows_spec(a, b=None, y=None):
    """where(y > 0, a + b, 0) over [M, C] rows; b = None: no second term; y = None: no gate.  A selection like
    relu_bwd_spec."""
    s = _f64(a) if b is None else _f64(a) + _f64(b)
    return s if y is None else torch.where(_f64(y) > 0, s, torch.zeros_like(s))


def add_gate_rows_f32(a, b=None, y=None, gate_ge=False, multiply=False):
    """Mutants as relu_bwd_f32."""
    s = a.float() if b is None else a.float() + b.float()
    return s if y is None else relu_bwd_f32(s, y, gate_ge, multiply)


def colsum_spec(x):
    """Column sums of x [M, C]: the bias gradient of a layer whose output gradient has the rows of x."""
    return _f64(x).sum(dim=0)


def colsum_f32(x, rows=None, fold4=False):
    """Mutants: `rows`, only the first `rows` rows are summed (a block's share dropped); `fold4`, for C < 4 column c takes
    component c of every float4 of the flat array, as the fold for C >= 4 would."""
    x = x.float()
    if fold4:
        assert x.shape[1] < 4 and x.numel() % 4 == 0
        return x.reshape(-1, 4).sum(dim=0)[:x.shape[1]]
    return (x if rows is None else x[:rows]).sum(dim=0)


def colsum_route(M, C, x_stride, ptr):
    """The kernel `colsum_f32` of csrc/train_ops.hip sends a call to, from its own conditions: "flat" (colsum_flat_kernel:
    dense, C a power of two <= 1024, M C a multiple of 4, 16-byte aligned) or "partial" (colsum_partial_kernel)."""
    flat = x_stride == C and C <= 1024 and C & (C - 1) == 0 and (M * C) % 4 == 0 and ptr % 16 == 0
    return "flat" if flat else "partial"


def mse_spec(a, b, g):
    """(value [1], da, db) of mean((a - b)^2) under the incoming scalar gradient g: da = 2 (a - b) g / n, db = -da."""
    d = _f64(a) - _f64(b)
    da = 2.0 * d * float(g) / d.numel()
    return d.pow(2).mean().reshape(1), da, -da


def mse_f32(a, b, g, two=2.0, count=None):
    """Mutants: `two` as in vq_bwd_f32; `count`, only the first `count` elements enter the sum (still divided by n)."""
    d = a.float() - b.float()
    n = d.numel()
    da = d * (torch.tensor(two, dtype=torch.float32) / float(n) * torch.tensor(float(g), dtype=torch.float32))
    return (d.reshape(-1)[:count].pow(2).sum() / float(n)).reshape(1), da, -da


def vq_finalize_spec(sse_part, counts, N, D):
    """(diff [1], perplexity [1]) (bottleneck.py:94, 97-100): diff = sum(sse_part) / (N D); perplexity =
    exp(-sum p log(max(p, 1e-7))), p = counts / N."""
    p = _f64(counts) / float(N)
    h = (p * torch.log(p.clamp(min=1e-7))).sum()
    return (_f64(sse_part).sum() / (float(N) * float(D))).reshape(1), torch.exp(-h).reshape(1)


def vq_finalize_f32(sse_part, counts, N, D, clamp=True):
    """Mutant: `clamp` = False, the logarithm of p itself (an unused code gives 0 * -inf)."""
    p = counts.float() / float(N)
    h = (p * torch.log(p.clamp(min=1e-7) if clamp else p)).sum()
    return (sse_part.float().sum() / (float(N) * float(D))).reshape(1), torch.exp(-h).reshape(1)


def ema_update_spec(embed, cluster_size, embed_avg, counts, embed_sum, decay, eps):
    """(embed', cluster_size', embed_avg') of the EMA codebook update (bottleneck.py:80-92), layout [D][K]:
    cs = decay cluster_size + (1 - decay) counts; ea = decay embed_avg + (1 - decay) embed_sum; n = sum(cs);
    embed' = ea / ((cs + eps) / (n + K eps) n).  decay and eps are the float32 values the C-ABI receives (`embed` itself is
    not read: the update replaces it)."""
    decay, eps = float(np.float32(decay)), float(np.float32(eps))
    cs = _f64(cluster_size) * decay + (1.0 - decay) * _f64(counts)
    ea = _f64(embed_avg) * decay + (1.0 - decay) * _f64(embed_sum)
    n = cs.sum()
    csn = (cs + eps) / (n + cs.shape[0] * eps) * n
    return ea / csn.unsqueeze(0), cs, ea


def ema_update_f32(embed, cluster_size, embed_avg, counts, embed_sum, decay, eps, n_codes=None):
    """Mutant: `n_codes`, only the first `n_codes` codes enter the total n."""
    decay, eps = torch.tensor(decay, dtype=torch.float32), torch.tensor(eps, dtype=torch.float32)
    cs = cluster_size.float() * decay + (1.0 - decay) * counts.float()
    ea = embed_avg.float() * decay + (1.0 - decay) * embed_sum.float()
    n = cs[:n_codes].sum()
    csn = (cs + eps) / (n + float(cs.shape[0]) * eps) * n
    return ea / csn.unsqueeze(0), cs, ea


def embed_code_spec(idx, codes, K):
    """out[n] = codes[clamp(idx[n], 0, K - 1)] for codes [K, D]: the documented clamp of an out-of-range index."""
    return _f64(codes)[torch.as_tensor(idx).cpu().long().reshape(-1).clamp(0, K - 1)]


def ema_state(D, K, gen, N=256):
    """A calibrated codebook state and one batch's statistics, float32: (embed [D, K], cluster_size [K], embed_avg =
    embed * cluster_size, counts [K], embed_sum [D, K]); both usage draws are peaked, so some codes are unused in
    either (cluster_size 0 with counts 0 gives embed' = 0 / (eps ...) = 0).  N, the vectors per batch, is small on purpose:
    embed' = ea / (cs + eps) * (1 + K eps / n) depends on the total n only through K eps / n, 8e-5 at K = 2048 and
    n = 256 but 5e-6 at n = 4096 -- a wrong total would hide under the comparison's floor at a large batch."""
    embed = torch.randn(D, K, generator=gen)
    w = torch.exp(-torch.arange(K, dtype=torch.float32) * (6.0 / K))
    w = w[torch.randperm(K, generator=gen)]
    cluster_size = torch.bincount(torch.multinomial(w, N, replacement=True, generator=gen), minlength=K).float()
    idx = torch.multinomial(w, N, replacement=True, generator=gen)
    counts = torch.bincount(idx, minlength=K).float()
    z = embed.t()[idx] + 0.1 * torch.randn(N, D, generator=gen)
    embed_sum = torch.zeros(K, D).index_add_(0, idx, z).t().contiguous()
    return embed, cluster_size, embed * cluster_size, counts, embed_sum


def gate_data(n, gen):
    """(dy, y) float32 [n] for a ReLU gate: y = randn with +0.0, -0.0, the smallest normal 2^-126 and negatives at the head,
    at the tail and throughout (no denormals); dy = randn with NaN, +inf and -inf at masked places (y <= 0) only."""
    y = torch.randn(n, generator=gen)
    special = torch.tensor([0.0, -0.0, 2.0 ** -126, -1.5, 3.0])
    where = torch.cat([torch.arange(min(n, 5)), torch.arange(5, max(n, 5), 13), torch.arange(max(n - 5, 0), n)])
    y[where] = special[where % 5]
    dy = torch.randn(n, generator=gen)
    masked = (y <= 0).nonzero().reshape(-1)
    for j, v in enumerate((float("nan"), float("inf"), float("-inf"))):
        dy[masked[j::4]] = v
    return dy, y


# ---------------------------------------------------------------------------------------------------------------------
# Float64 specification, float32 yardstick and split-product models of the convolution weight gradients
# (csrc/conv_wgrad_f32.hip), in the style of the row-ops block above: plain torch on the CPU, no autograd and none of the
# project's kernels.  A weight gradient is an im2col contraction over pixels,
#     dW2d[r][c] = sum over (b, l) of rows[b][l][r] * cols[b][c][l],
# with, for a plain convolution, rows = dY [B, OH OW, Cout] and cols = unfold(zero-padded cat(x, x2)) [B, Cin k k, OH OW]:
#     dW[co, ci, kh, kw] = sum_{b, oy, ox} dY[b, oy, ox, co] * xpad[b, ci, oy s + kh, ox s + kw],
# and for ConvTranspose2d(4, 2, 1) rows = x [B, H W, Cin] and cols = unfold(dY, 4, padding 1, stride 2) [B, Cout 16, H W]:
#     dW[ci, co, kh, kw] = sum_{b, iy, ix} x[b, ci, iy, ix] * dY[b, co, 2 iy - 1 + kh, 2 ix - 1 + kw]   (out of range: dropped).
# db is the column sum of dY.  A "row" for compare_rows is one output channel's gradient: reshape dW to [rows, -1].
# tests/test_conv_wgrad_host.py holds the spec to float64 autograd and shows what the comparison rejects;
# tests/test_conv_wgrad_gpu.py holds the kernels to it.
def _wgrad_operands(x, x2, dy_nhwc, k, stride, pad, transposed, dtype, clamp_border=False, swap_sources=False):
    """(rows [B, L, R], cols [B, Ccols, L], dY as [B L', Cout]) of the contraction above in `dtype`.  The two switches are the
    host tests' mutants: `clamp_border` replicates the border instead of zero padding, `swap_sources` concatenates (x2, x)."""
    x, dy = torch.as_tensor(x).detach().cpu().to(dtype), torch.as_tensor(dy_nhwc).detach().cpu().to(dtype)
    if x2 is not None:
        x2 = torch.as_tensor(x2).detach().cpu().to(dtype)
        x = torch.cat([x2, x] if swap_sources else [x, x2], dim=1)
    B = x.shape[0]
    dy2d = dy.reshape(-1, dy.shape[-1])
    if transposed:
        assert (k, stride, pad) == (4, 2, 1) and x2 is None
        src, rows = dy.permute(0, 3, 1, 2), x.permute(0, 2, 3, 1).reshape(B, -1, x.shape[1])
    else:
        src, rows = x, dy.reshape(B, -1, dy.shape[-1])
    if clamp_border and pad:
        src, pad = torch.nn.functional.pad(src, (pad,) * 4, mode="replicate"), 0
    cols = torch.nn.functional.unfold(src, k, padding=pad, stride=stride)
    assert cols.shape[2] == rows.shape[1], (cols.shape, rows.shape)
    return rows, cols, dy2d


def _wgrad_shape(dw2d, k, groups):
    """[R, C k k] -> torch's weight layout [R, C / groups, k, k]: the block-diagonal part of the dense gradient."""
    R = dw2d.shape[0]
    dw = dw2d.reshape(R, -1, k, k)
    if groups == 1:
        return dw
    r, c = R // groups, dw.shape[1] // groups
    return torch.cat([dw[g * r:(g + 1) * r, g * c:(g + 1) * c] for g in range(groups)], 0)


def _wgrad_contract(rows, cols, pixels=None):
    if pixels is not None:                                # the pixels (b, l) that are summed, as a flat boolean mask
        rows = rows * pixels.reshape(rows.shape[0], -1, 1).to(rows.dtype)
    return torch.einsum("blr,bcl->rc", rows, cols)


def conv_wgrad_spec(x, x2, dy_nhwc, k, stride, pad, transposed, groups=1):
    """(dW in torch's layout, db) in float64: Conv2d [Cout, Cin / groups, k, k], ConvTranspose2d [Cin, Cout / groups, 4, 4]."""
    rows, cols, dy2d = _wgrad_operands(x, x2, dy_nhwc, k, stride, pad, transposed, torch.float64)
    return _wgrad_shape(_wgrad_contract(rows, cols), k, groups), dy2d.sum(dim=0)


def conv_wgrad_f32_yardstick(x, x2, dy_nhwc, k, stride, pad, transposed, groups=1, pixels=None, db_pixels=None,
                             clamp_border=False, swap_sources=False, x_hi_only=False):
    """The same contraction in float32 on the CPU: what float32 can do on that data.  The switches are the host tests' mutants:
    `pixels` / `db_pixels` (flat boolean masks over the summed pixels) drop pixels from dW / db, `clamp_border`,
    `swap_sources` (see _wgrad_operands), `x_hi_only` carries the layer input as its bf16 hi piece alone."""
    rows, cols, dy2d = _wgrad_operands(x, x2, dy_nhwc, k, stride, pad, transposed, torch.float32, clamp_border, swap_sources)
    if x_hi_only:
        if transposed:
            rows = rows.bfloat16().float()
        else:
            cols = cols.bfloat16().float()
    db = dy2d.sum(dim=0) if db_pixels is None else (dy2d * db_pixels.reshape(-1, 1).float()).sum(dim=0)
    return _wgrad_shape(_wgrad_contract(rows, cols, pixels), k, groups), db


def bf16_pieces(v, pieces):
    """The split of csrc/conv_wgrad_f32.hip::split4<NP> on a float32 tensor, as float64 tensors: NP = 2: (hi, lo) with
    hi = rne_bf16(v), lo = rne_bf16(v - hi); NP = 3: (hi, mid, lo) with mid = rne_bf16(v - hi), lo = rne_bf16(v - hi - mid)
    (the subtractions are exact in float32, so v = hi + mid + lo exactly)."""
    v = v.float()
    rne = lambda t: t.bfloat16().float()
    hi = rne(v)
    r = v - hi
    if pieces == 2:
        return hi.double(), rne(r).double()
    assert pieces == 3
    mid = rne(r)
    return hi.double(), mid.double(), rne(r - mid).double()


def conv_wgrad_split_model(x, x2, dy_nhwc, k, stride, pad, transposed, pieces, groups=1, drop_lo=False):
    """Float64 evaluation of the products the split-bf16 kernels document: its distance from conv_wgrad_spec is the truncation
    a precision mode accepts by design.  Every element of dY (D) and of the im2col operand (X) is split by `bf16_pieces` and
    the sum runs over the terms the kernel keeps.  conv_wgrad_split_kernel<NP> (piece index 0 hi, 1 lo, 2 mid; term(qa, qb)
    multiplies piece qa of dY with piece qb of the input):
        } else if constexpr (NP == 3) {   // smallest terms first: lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi
          term(1, 0); term(0, 1); term(2, 2); term(2, 0); term(0, 2); term(0, 0);
        } else {
          term(1, 0); term(0, 1); term(0, 0);
    so pieces = 2 keeps D.hi X.hi + D.hi X.lo + D.lo X.hi and pieces = 3 those plus D.hi X.mid + D.mid X.hi + D.mid X.mid (with
    the three-piece lo).  conv_wgrad_halo_kernel stages both operands with split4<2> and issues
        mfma(al, bh[c]) ; mfma(ah, bl[c]) ; mfma(ah, bh[c])
    the same three terms as pieces = 2.  A pair-format source (x_pair) is decoded first -- "the staging decodes (hi + lo) / 4 --
    exactly the value the forward's products saw" -- and that float32 value is split into bf16 pieces like any other: model it
    by passing `pair_round_f16(x)` as the input, with pieces = 2.  The one-hot form (vq_embed_sum) keeps D.lo, D.mid, D.hi
    against an operand that is exact in its hi piece, i.e. the exact float32 terms: its yardstick is the float32 evaluation.
    `drop_lo` is a host-test mutant: the lo piece of both operands is left out."""
    rows, cols, _ = _wgrad_operands(x, x2, dy_nhwc, k, stride, pad, transposed, torch.float32)
    R, Cc = bf16_pieces(rows, pieces), bf16_pieces(cols, pieces)
    if pieces == 2:
        hi, lo = 0, 1
        terms = [(hi, hi), (hi, lo), (lo, hi)]
    else:
        hi, mid, lo = 0, 1, 2
        terms = [(hi, hi), (hi, mid), (mid, hi), (mid, mid), (hi, lo), (lo, hi)]
    if drop_lo:
        terms = [t for t in terms if lo not in t]
    # (which operand is dY and which the input differs between the plain and the transposed form; the term list is symmetric)
    dw = sum(_wgrad_contract(R[a], Cc[b]) for a, b in terms)
    return _wgrad_shape(dw, k, groups)


def pair_round_f16(x):
    """The float32 value a split-f16 pair holds (csrc/split_f16.h: x s = hi + lo, hi = f16(x s), lo = f16(x s - hi), s = 4):
    (hi + lo) / 4."""
    xs = x.float() * 4.0
    hi = xs.half().float()
    return (hi + (xs - hi).half().float()) / 4.0


def larger_error(a, b, ref):
    """Element-wise, whichever of a and b lies further from ref: as a yardstick, its row error is the larger of the two's."""
    a, b, ref = _f64(a), _f64(b), _f64(ref)
    return torch.where((a - ref).abs() >= (b - ref).abs(), a, b)


# The six-term mode (flags 4) keeps the project's margin of 8 although its yardstick, the float64 evaluation of the six kept
# terms, prices the truncation only (~1e-8 of a row: the bound is the floor, 8 x 2^-23, whatever the number of pixels), while
# the kernel accumulates 6 M products in ONE float32 accumulator per split -- per 32-pixel chunk two steps of six MFMA each,
# every one rounding the running sum: about 12 M / 32 roundings of 2^-24 of the row's scale, ~sqrt(12 M / 32) 2^-24.  The cases
# below keep a split at or under 352 pixels, where that is within the bound: the largest ratio measured on the MI355X is 7.0
# (128 x 128 tile, M = 666 in two splits; profiles/wgrad_checks.txt), the exact-fp32 kernel and the float32 evaluation on
# the CPU sitting at 3.6 and 6.4 floors on the same data for the same reason.  A longer split would need a yardstick that
# prices the accumulation (the float32 evaluation, as for flags 2), not a wider margin.
def wgrad_split_tile(rows, K):
    """The tile `wgrad_tile` of csrc/conv_wgrad_f32.hip selects for a [rows][K] gradient (rows = the GEMM's output channels)."""
    Kpad = (K + 31) // 32 * 32
    if Kpad <= 64:
        return "64x64" if rows <= 64 else "128x64"
    return "32x512" if rows <= 32 else "128x128"


def wgrad_case_tile(c):
    """Tile of a case: a transposed layer runs with the roles swapped (rows = its input channels, K = 16 x its output
    channels, those padded to 4 when fewer), a source of fewer than 4 channels is padded to 4."""
    if c.transposed:
        return wgrad_split_tile(c.c0, 16 * max(c.cout, 4))
    cin = c.c0 + c.c1
    return wgrad_split_tile(c.cout, c.k * c.k * (4 if cin < 4 and not c.c1 else cin))


def conv_wgrad_yardstick(flags, spec_dw, f32_dw, model2_dw=None, model3_dw=None):
    """The yardstick of a precision mode (the flag bits of isi_conv_wgrad_f32): 0 (and every launch that runs the fp32 pipe):
    the float32 evaluation; 2 (three-term products): per element the worse of the float32 evaluation and the pieces = 2
    model; 4 (six-term): the pieces = 3 model."""
    if flags == 0:
        return f32_dw
    if flags == 2:
        return larger_error(f32_dw, model2_dw, spec_dw)
    assert flags == 4
    return model3_dw


# ConvTranspose2d(4, 2, 1) as four stride-1 2x2 convolutions, one per output phase (py, px) = (oy % 2, ox % 2): the form of
# isi_conv_wgrad_f32 with bit 0 of its flag word set.  Phase p = 2 py + px, tap (ty, tx) reads the input at
# (oy - (1 - py) + ty, ox - (1 - px) + tx) and is torch's tap (ky, kx) = (3 - py - 2 ty, 3 - px - 2 tx) (csrc/pack.hip).
def convT_phases_f32(x, dy_nhwc, pad_of=lambda p: 1 - p, dtype=torch.float32):
    """Packed [4][Cout][4 Cin] (k = (ty 2 + tx) Cin + ci) weight gradient of the four-phase form.  `pad_of` (phase bit -> top /
    left padding) is the host tests' mutant switch: the kernel's is 1 - p."""
    x = torch.as_tensor(x).detach().cpu().to(dtype)
    dy = torch.as_tensor(dy_nhwc).detach().cpu().to(dtype)
    B, Cin, H, W = x.shape
    Cout = dy.shape[-1]
    out = torch.zeros(4, Cout, 4 * Cin, dtype=dtype)
    for py in range(2):
        for px in range(2):
            dyp = dy[:, py::2, px::2, :].reshape(B, H * W, Cout)
            pt, pl = pad_of(py), pad_of(px)
            xp = torch.nn.functional.pad(x, (pl, 1 - pl, pt, 1 - pt))                        # [B, Cin, H + 1, W + 1]
            cols = torch.nn.functional.unfold(xp, 2).reshape(B, Cin, 4, H * W)               # [b][ci][ty 2 + tx][l]
            out[2 * py + px] = torch.einsum("blo,bctl->otc", dyp, cols).reshape(Cout, 4 * Cin)
    return out


def convT_unpack_phases(packed, Cin, Cout):
    """[4][Cout][>= 4 Cin] packed phase gradients -> torch's ConvTranspose2d layout [Cin, Cout, 4, 4]."""
    packed = torch.as_tensor(packed).detach().cpu()
    dw = torch.zeros(Cin, Cout, 4, 4, dtype=packed.dtype)
    for py in range(2):
        for px in range(2):
            m = packed[2 * py + px][:, :4 * Cin].reshape(Cout, 2, 2, Cin)
            for ty in range(2):
                for tx in range(2):
                    dw[:, :, 3 - py - 2 * ty, 3 - px - 2 * tx] = m[:, ty, tx, :].t()
    return dw


def embed_sum_spec(z, idx, K):
    """embed_sum [D, K] = z^T @ one_hot(idx) in float64, as an index_add over the rows of z [N, D]."""
    z = _f64(z)
    out = torch.zeros(K, z.shape[1], dtype=torch.float64)
    out.index_add_(0, torch.as_tensor(idx).cpu().long().reshape(-1), z)
    return out.t().contiguous()


def embed_sum_f32(z, idx, K):
    z = torch.as_tensor(z).detach().cpu().float()
    out = torch.zeros(K, z.shape[1], dtype=torch.float32)
    out.index_add_(0, torch.as_tensor(idx).cpu().long().reshape(-1), z)
    return out.t().contiguous()


# The cases of both weight-gradient test files.  route: the kernel family the dispatcher of conv_wgrad_batched_f32 sends the
# case to under three-term products (flags 2); c1: channels of a second source (0: one source); layout of the layer input:
# "nhwc" dense channels-last, "nchw" dense NCHW (not vectorisable: scalar gather), "pair" split-f16 pair tensors;
# B, H, W: the layer INPUT.  `vec`: the operands are vectorisable (Cin % 4 == 0 per source, Cout % 4 == 0, channels-last), so
# the precision bits select the kernel; otherwise the fp32 pipe runs whatever the flags.
WgradCase = collections.namedtuple("WgradCase", "route c0 c1 cout k stride pad transposed groups B H W layout vec")


def _wc(route, c0, c1, cout, k, stride, pad, B, H, W, transposed=False, groups=1, layout="nhwc", vec=True):
    return WgradCase(route, c0, c1, cout, k, stride, pad, transposed, groups, B, H, W, layout, vec)


WGRAD_CASES = [
    # halo-staged kernel: 3x3 s1 p1 / k4 s2 p1, 32-multiple channels, OW % 32 == 0, OH % 2 == 0.  One 2 x 32 tile: ntiles / 4 = 0
    # so one split; nco = 4 (Cout % 128 == 0), 2 (Cout % 64 == 0), 1
    _wc("halo", 128, 0, 128, 3, 1, 1, 1, 2, 32), _wc("halo", 64, 0, 64, 3, 1, 1, 1, 2, 32), _wc("halo", 128, 0, 32, 3, 1, 1, 1, 2, 32),
    # 12 tiles, 4 units: min(256 / 4, 12 / 4) = 3 splits of 4 tiles; 14 tiles: 3 splits of 5, 5 and 4
    _wc("halo", 128, 0, 128, 3, 1, 1, 3, 4, 64), _wc("halo", 128, 0, 128, 3, 1, 1, 7, 2, 64),
    _wc("halo", 64, 0, 128, 4, 2, 1, 1, 4, 64),                                              # k4 s2: both tap groups
    _wc("halo", 128, 0, 128, 3, 1, 1, 2, 4, 32, layout="pair"), _wc("halo", 32, 32, 128, 3, 1, 1, 2, 4, 32, layout="pair"),
    # the same three layers one column / one row off the halo kernel's whole tiles: OW % 32 != 0 or OH % 2 != 0 -> split kernel
    *[_wc("split", ci, 0, co, 3, 1, 1, 1, h, w) for ci, co in ((128, 128), (64, 64), (128, 32)) for h, w in ((2, 33), (2, 31), (3, 32))],
    # split 128 x 128 (Kpad > 64, Cout > 32).  M = 666: 21 chunks of 32 pixels, nsplit = min(768 / 5 tiles, 21 / 8) = 2 splits of
    # 11 and 10 chunks, the last chunk 26 pixels
    _wc("split", 64, 0, 128, 3, 1, 1, 2, 9, 37), _wc("split", 64, 64, 128, 3, 1, 1, 2, 9, 37),
    # split 32 x 512 (Cout <= 32), Cout below the tile; M = 5 < 32
    _wc("split", 128, 0, 32, 3, 1, 1, 2, 9, 37), _wc("split", 128, 0, 8, 3, 1, 1, 2, 9, 37),
    _wc("split", 128, 0, 32, 3, 1, 1, 1, 1, 5), _wc("split", 128, 0, 8, 3, 1, 1, 1, 1, 5),
    _wc("split", 32, 0, 128, 1, 1, 0, 2, 9, 37),                                             # split 128 x 64: K = 32 = Kpad <= 64
    # split 64 x 64 (Kpad <= 64, Cout <= 64): the 2-channel side through isi_pad_channels4_f32, cin_keep = 2; M = 342 and M = 1
    _wc("split", 2, 0, 32, 4, 2, 1, 2, 18, 38), _wc("split", 2, 0, 64, 4, 2, 1, 2, 18, 38),
    _wc("split", 2, 0, 32, 4, 2, 1, 1, 2, 2), _wc("split", 2, 0, 64, 4, 2, 1, 1, 2, 2),
    # K % 32 != 0: K = 72 -> Kpad = 96, K = 108 -> Kpad = 128 (split 32 x 512; M = 35)
    _wc("split", 8, 0, 16, 3, 1, 1, 1, 5, 7), _wc("split", 12, 0, 16, 3, 1, 1, 1, 5, 7),
    # scalar gather of conv_wgrad_f32_kernel (fp32 pipe whatever the flags): Cin % 4 != 0 (quads straddle taps); Cout % 4 != 0
    # (dvec = 0); an NCHW source; two sources with C0 = 6 (quads straddle the sources)
    *[_wc("scalar", ci, c1, co, 3, 1, 1, B, H, W, layout=lay, vec=False)
      for B, H, W in ((1, 5, 7), (2, 9, 37)) for ci, c1, co, lay in ((6, 0, 16, "nhwc"), (64, 0, 6, "nhwc"), (64, 0, 64, "nchw"), (6, 10, 16, "nhwc"))],
    # ConvTranspose2d through vqvae/_train.py conv_wgrad: the adjoint stride-2 convolution with the roles swapped (source = dY,
    # a channel slice of a wider gradient; 2 and 1 channels go through isi_pad_channels4_f32), db by isi_colsum_f32
    *[_wc("split", ci, 0, co, 4, 2, 1, B, H, W, transposed=True) for B, H, W in ((1, 3, 5), (2, 9, 19)) for ci, co in ((128, 64), (64, 2), (32, 1))],
    _wc("split", 32, 0, 32, 3, 1, 1, 1, 5, 7, groups=2),                                     # layer.grouped(...) of the dense gradient
]
# the four-phase transposed C entry (bit 0 of isi_conv_wgrad_f32's flag word): (Cin, Cout, B, H, W, vectorisable)
WGRAD_PHASE_CASES = [(32, 64, 1, 3, 5, True), (32, 64, 2, 9, 19, True), (6, 8, 1, 3, 5, False), (6, 8, 2, 9, 19, False)]


def wgrad_case_id(c):
    src = f"{c.c0}+{c.c1}" if c.c1 else f"{c.c0}"
    return (f"{c.route}-{'convT' if c.transposed else 'conv'}{src}to{c.cout}k{c.k}s{c.stride}p{c.pad}"
            f"{'g%d' % c.groups if c.groups > 1 else ''}-{c.B}x{c.H}x{c.W}-{c.layout}")


def wgrad_case_data(c):
    """(x [B, C0, H, W], x2 or None, dy [B, OH, OW, Cout]) float32 on the CPU: seeded randn, the layer input rectified as the
    forward rectifies it (roughly half zeros), pair-format sources rounded to what their pairs hold."""
    seed = 0
    for v in (c.c0, c.c1, c.cout, c.k, c.stride, c.pad, int(c.transposed), c.groups, c.B, c.H, c.W, ("nhwc", "nchw", "pair").index(c.layout)):
        seed = (seed * 131 + v) % (2 ** 31 - 1)
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(c.B, c.c0, c.H, c.W, generator=g))
    x2 = torch.relu(torch.randn(c.B, c.c1, c.H, c.W, generator=g)) if c.c1 else None
    if c.transposed:
        OH, OW = 2 * c.H, 2 * c.W
    else:
        OH, OW = (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1
    dy = torch.randn(c.B, OH, OW, c.cout, generator=g)
    if c.layout == "pair":
        x, x2 = pair_round_f16(x), (pair_round_f16(x2) if x2 is not None else None)
    return x, x2, dy


def wgrad_phase_case_data(shape):
    """(x [B, Cin, H, W] rectified, dy [B, 2H, 2W, Cout]) of a WGRAD_PHASE_CASES entry, float32 on the CPU."""
    cin, cout, B, H, W, _ = shape
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + B)
    return torch.relu(torch.randn(B, cin, H, W, generator=g)), torch.randn(B, 2 * H, 2 * W, cout, generator=g)


WgradRefs = collections.namedtuple("WgradRefs", "spec_dw spec_db f32_dw f32_db model2 model3")
_wgrad_refs_cache = {}


def wgrad_case_refs(c):
    """The spec, the float32 yardstick and the two split models of a case, computed once per process and left unchanged
    (the models only where the precision bits can select a split kernel)."""
    if c not in _wgrad_refs_cache:
        x, x2, dy = wgrad_case_data(c)
        a = (x, x2, dy, c.k, c.stride, c.pad, c.transposed)
        spec_dw, spec_db = conv_wgrad_spec(*a, groups=c.groups)
        f32_dw, f32_db = conv_wgrad_f32_yardstick(*a, groups=c.groups)
        m2 = conv_wgrad_split_model(*a, pieces=2, groups=c.groups) if c.vec else None
        m3 = conv_wgrad_split_model(*a, pieces=3, groups=c.groups) if c.vec else None
        _wgrad_refs_cache[c] = WgradRefs(spec_dw, spec_db, f32_dw, f32_db, m2, m3)
    return _wgrad_refs_cache[c]


def rows2d(t):
    """A weight gradient as [rows, -1] (a row = one output channel's gradient); vectors stay vectors."""
    return t.reshape(t.shape[0], -1) if t.dim() > 1 else t


# ---------------------------------------------------------------------------------------------------------------------
# Float64 specification, float32 yardstick and split-product models of the linear layers' GEMM (csrc/gemm_split_f32.hip,
# through isi_linear_f32), in the style of the blocks above: plain torch, no autograd and none of the project's kernels.
#     v = x W^T + bias + res;  ReLU;  gate > 0 ? v * gate_scale : 0;  keep ? v / (1 - p) : 0          (the epilogue's order)
# with W [N, K] in torch's layout, `gate_scale` and `p` the float32 values the C-ABI receives, and `keep` the mask of
# `dropout_keep_mask`.  Everything here computes on the device its operands live on (the CPU, except for the two shapes of
# 8 M and 16 M outputs that tests/test_linear_gemm_gpu.py needs to reach the 256-row tiles: torch's matmuls, not the
# project's).  tests/test_linear_gemm_host.py holds the spec to float64 autograd and shows what `linear_hold` rejects;
# tests/test_linear_gemm_gpu.py holds the kernels to it on every tile route.
LINEAR_TAIL_ROWS = 16          # kGemmTailRows: M % 128 up to this many rows (of M >= 1024) are fp32 dot products, no tile row
LINEAR_TILES = {1: "128x64", 2: "128x128", 3: "256x128", 4: "256x256"}


def linear_route(M, N, K, cus, narrow_below=0, no_wide=0):
    """Mirror of gemm_split_route / isi_linear_route (csrc/gemm_split_f32.hip) for a device of `cus` compute units and the
    knobs ISI_GEMM_NARROW_BELOW / ISI_GEMM_NO_WIDE: 0 = outside the GEMM kernel, else tile | tail_rows << 8 (LINEAR_TILES)."""
    if K % 32 or K < 128 or N <= 32 or M < 256:
        return 0
    tail, rem = 0, M % 128
    if 0 < rem <= LINEAR_TAIL_ROWS and M >= 8 * 128:
        tail, M = rem, M - rem
    cdiv = lambda a, b: (a + b - 1) // b
    narrow = cdiv(M, 128) * cdiv(N, 128) < (narrow_below if narrow_below > 0 else cus) or N % 128 != 0
    if narrow:
        tile = 1
    elif N % 256 == 0 and cdiv(M, 256) * cdiv(N, 256) == cus and not no_wide:
        tile = 4
    elif (cdiv(M, 256) * cdiv(N, 128)) % cus == 0 and no_wide != 1:
        tile = 3
    else:
        tile = 2
    return tile | tail << 8


def dropout_thresh(p):
    """The 32-bit threshold of gemm_split_f32: (double)(float)p * 2^32, truncated, clamped to [1, 0xFFFFFFFF]."""
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else 1 if t < 1.0 else int(t)


def dropout_keep_mask(seed, M, N, ldo, p, high_word=True):
    """Integer replica of `dropout_keep` (csrc/isi_internal.h) over an [M, N] output of row stride ldo, as a bool tensor: the
    lowbias32 mixer over idx = m ldo + n (32 bits), the seed's low word folded in after round one and the high word inside
    round two, in front of its multiply; keep iff h >= thresh.  `high_word` = False is a host-test mutant (the seed's high word ignored)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(ldo) + np.arange(N, dtype=np.uint64)[None, :]
    h = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7FEB352D)
    h ^= np.uint32(seed & 0xFFFFFFFF)
    h ^= h >> np.uint32(15)
    if high_word:
        h ^= np.uint32(seed >> 32)
    h *= np.uint32(0x846CA68B)
    h ^= h >> np.uint32(16)
    return torch.from_numpy(h >= np.uint32(dropout_thresh(p)))


def _linear_epilogue(v, bias, res, relu, gate, gate_scale, keep, p, gate_ge=False, gate_unscaled=False,
                     keep_unscaled=False):
    """The epilogue in v's dtype on v's device; returns (out, lin, live): `lin` the value without the ReLU (scaled like
    `out`), `live` where neither the gate nor the mask forces a zero (None: everywhere)."""
    to = lambda t: torch.as_tensor(t).detach().to(device=v.device, dtype=v.dtype)
    if bias is not None:
        v = v + to(bias)
    if res is not None:
        v = v + to(res)
    lin, live = v, None
    if gate is not None:
        gs = torch.tensor(1.0 if gate_unscaled else float(np.float32(gate_scale)), dtype=v.dtype, device=v.device)
        g = torch.as_tensor(gate).detach().to(v.device)
        live = (g >= 0) if gate_ge else (g > 0)
        lin = lin * gs
    if keep is not None:
        k = torch.as_tensor(keep).to(v.device)
        live = k if live is None else live & k
        if not keep_unscaled:
            lin = lin / (1.0 - torch.tensor(float(np.float32(p)), dtype=v.dtype, device=v.device))
    out = lin.clamp(min=0.0) if relu else lin
    if live is not None:
        out = torch.where(live, out, torch.zeros_like(out))
    return out, lin, live


def linear_spec(x, W, bias, res, relu, gate=None, gate_scale=1.0, keep=None, p=0.0, prod=None, parts=False):
    """Float64 closed form of isi_linear_f32.  `prod`: the float64 product x W^T where the caller has it already (one per
    case, every epilogue on top of it); `parts`: return (out, lin, live) of _linear_epilogue, not out alone."""
    if prod is None:
        prod = torch.as_tensor(x).detach().double() @ torch.as_tensor(W).detach().double().t()
    r = _linear_epilogue(prod.double(), bias, res, relu, gate, gate_scale, keep, p)
    return r if parts else r[0]


def linear_f32(x, W, bias, res, relu, gate=None, gate_scale=1.0, keep=None, p=0.0, prod=None, skip_last_chunk=False,
               repeat_chunk=False, x_dense=None, res_dense=None, tail_bf16=False, **epilogue_mutants):
    """The same in float32 torch: the yardstick of the tail rows, half of the tile rows', and what the host tests apply
    their mutants to.  `prod`: the float32 product where the caller has it.  Mutants: `skip_last_chunk`, the last 32 k
    left out; `repeat_chunk`, the next-to-last 32 k of both operands in place of the last; `x_dense` = (flat buffer, first
    element): rows of x read at stride K from there, not at their stride; `res_dense` likewise for the residual at stride N;
    `tail_bf16`, single-term bf16 products (operands rounded to bf16); gate_ge / gate_unscaled / keep_unscaled: the epilogue's."""
    if prod is None:
        xf, Wf = torch.as_tensor(x).detach().float(), torch.as_tensor(W).detach().float()
        M, K = xf.shape
        if x_dense is not None:
            buf, first = x_dense
            xf = buf.reshape(-1)[first:first + M * K].reshape(M, K).float()
        if tail_bf16:
            xf, Wf = xf.bfloat16().float(), Wf.bfloat16().float()
        if skip_last_chunk:
            xf, Wf = xf[:, :K - 32], Wf[:, :K - 32]
        elif repeat_chunk:
            xf = torch.cat([xf[:, :K - 32], xf[:, K - 64:K - 32]], dim=1)
            Wf = torch.cat([Wf[:, :K - 32], Wf[:, K - 64:K - 32]], dim=1)
        prod = xf @ Wf.t()
    if res_dense is not None:
        buf, first = res_dense
        res = buf.reshape(-1)[first:first + prod.numel()].reshape(prod.shape)
    return _linear_epilogue(prod.float(), bias, res, relu, gate, gate_scale, keep, p, **epilogue_mutants)[0]


def f16_pieces(v, scale):
    """The split of csrc/split_f16.h on a float32 tensor, as float64 tensors: hi = f16(s v), lo = f16(s v - hi) (the product
    by the power of two s and the subtraction are exact in float32)."""
    sv = v.float() * scale
    hi = sv.half().float()
    return hi.double(), (sv - hi).half().double()


def linear_split_model(x, W, mode, drop=None):
    """Float64 evaluation of the three terms gemm_split_kernel keeps of x W^T -- mfma(al, bh); mfma(ah, bl); mfma(ah, bh):
    lo.hi + hi.lo + hi.hi -- with the pieces of its product mode: "bf16" (ISI_CONV_BF16X3): bf16_pieces(v, 2) of both
    operands; "f16" (ISI_CONV_F16X3): f16_pieces of 4 x and 1024 W, the sum divided by 4096.  Its distance from the exact
    product is the truncation the mode accepts by design.  `drop` ("hi_lo" or "lo_hi": x piece, W piece) is a host-test
    mutant: that cross term is left out."""
    x, W = torch.as_tensor(x).detach(), torch.as_tensor(W).detach()
    if mode == "bf16":
        (xh, xl), (wh, wl), unscale = bf16_pieces(x, 2), bf16_pieces(W, 2), 1.0
    else:
        assert mode == "f16", mode
        (xh, xl), (wh, wl), unscale = f16_pieces(x, 4.0), f16_pieces(W, 1024.0), 1.0 / 4096.0
    s = xh @ wh.t()
    if drop != "hi_lo":
        s = s + xh @ wl.t()
    if drop != "lo_hi":
        s = s + xl @ wh.t()
    assert drop in (None, "hi_lo", "lo_hi"), drop
    return s * unscale


def _larger_error_on(a, b, ref):
    """larger_error on the device of ref."""
    a, b = a.to(ref.device).double(), b.to(ref.device).double()
    return torch.where((a - ref).abs() >= (b - ref).abs(), a, b)


LinearExpect = collections.namedtuple("LinearExpect", "spec lin live yard relu tail")


def linear_expect(prod64, prod32, model, tail, bias, res, relu, gate=None, gate_scale=1.0, keep=None, p=0.0):
    """What one launch is held to: the spec on top of the float64 product, and the yardstick -- for the tile rows (all but
    the last `tail`) per element the worse of the float32 evaluation and the mode's three-term model, for the tail rows
    (plain fp32 dot products in the kernel) the float32 evaluation alone -- every one with the same epilogue."""
    e = (bias, res, relu, gate, gate_scale, keep, p)
    spec, lin, live = linear_spec(None, None, *e, prod=prod64, parts=True)
    f32 = linear_f32(None, None, *e, prod=prod32)
    yard = _larger_error_on(f32, _linear_epilogue(model.double(), *e)[0], spec)
    if tail:
        yard[-tail:] = f32[-tail:].to(yard.device).double()
    return LinearExpect(spec, lin, live, yard, bool(relu), tail)


def linear_hold(got, exp, what, margin=ROW_OPS_MARGIN):
    """The comparison of the linear-GEMM tests, tile rows and tail rows as blocks of their own.  Per block:
      * zeros: an element the gate or the mask removes is 0 exactly; with the ReLU, so is one whose float64 value lies more
        than `tol` below 0; every other element further than `tol` from 0 is not 0 -- tol = what compare_rows allows that
        row, margin x yardstick error x the row's largest |spec| (an element nearer 0 than the kernel may be wrong by can
        fall on either side of a ReLU);
      * values: compare_rows over the whole block, zeros included.
    Returns the RowChecks; raises AssertionError at the first failure."""
    M = exp.spec.shape[0]
    got = torch.as_tensor(got).detach().to(exp.spec.device)
    assert got.shape == exp.spec.shape, f"{what}: shape {tuple(got.shape)} against {tuple(exp.spec.shape)}"
    checks = []
    for name, rows in (("tile rows", slice(0, M - exp.tail)), ("tail rows", slice(M - exp.tail, M))):
        if rows.start == rows.stop:
            continue
        g, spec, lin, yard = got[rows], exp.spec[rows], exp.lin[rows], exp.yard[rows]
        live = torch.ones_like(spec, dtype=torch.bool) if exp.live is None else exp.live[rows]
        yerr = max(row_error(yard, spec), ROW_OPS_FLOOR)
        tol = margin * yerr * spec.abs().amax(dim=-1, keepdim=True).clamp(min=2.0 ** -100)
        must_zero = ~live | (lin < -tol if exp.relu else torch.zeros_like(live))
        must_not = live & ((lin > tol) if exp.relu else (lin.abs() > tol))
        bad0, bad1 = int((g[must_zero] != 0).sum()), int((g[must_not] == 0).sum())
        assert bad0 == 0, f"{what} {name}: {bad0} of {int(must_zero.sum())} elements the spec zeroes are not 0"
        assert bad1 == 0, f"{what} {name}: {bad1} of {int(must_not.sum())} elements the spec keeps are 0"
        checks.append(compare_rows(g, spec, yard, f"{what} {name}", margin))
    return checks


def linear_case_data(M, N, K, seed=None):
    """(x [M, K], W [N, K] = randn / sqrt(K), bias [N], res [M, N], gate [M, N]) float32 on the CPU, seeded by the shape; the
    gate is `gate_data`'s y: randn with +0.0, -0.0, 2^-126 and negatives at the head, at the tail and throughout."""
    g = torch.Generator().manual_seed((M * 131 + N) * 131 + K if seed is None else seed)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    gate = gate_data(M * N, g)[1].reshape(M, N)
    return x, W, bias, res, gate


LinearCase = collections.namedtuple("LinearCase", "M N K tile tail knobs")      # knobs: ((name, value), ...)
LINEAR_DROP_P = 0.25
LINEAR_SEEDS = ((0x9E3779B9 << 32) | 0x7F4A7C15, (0x0000002A << 32) | 0x7F4A7C15)     # above 2^32; they share the low word
LINEAR_EPILOGUES = ("bias", "bias+res+relu", "gate", "relu+dropout", "all")


def linear_cases(cus):
    """The cases of tests/test_linear_gemm_gpu.py for a device of `cus` compute units (the routes in the comments: 256), as
    (small, wide): below 1 M outputs every epilogue of LINEAR_EPILOGUES runs, at the wide shapes -- the smallest that reach the
    256-row tiles, which want a whole round of the chip -- the first and the last."""
    nb = (("ISI_GEMM_NARROW_BELOW", 1),)
    small = [
        # 128 x 64, default knobs: ragged N below one tile, one row past a tile, K of 4 and of 5 chunks (both parities of the
        # two-stage ring, the peeled last chunk)
        LinearCase(256, 40, 128, 1, 0, ()), LinearCase(257, 72, 160, 1, 0, ()), LinearCase(300, 200, 128, 1, 0, ()),
        # ... with tail rows: 6, the most (16), and one more (17 rows take a tile of their own)
        LinearCase(1030, 192, 128, 1, 6, ()), LinearCase(1040, 64, 128, 1, 16, ()), LinearCase(1041, 64, 128, 1, 0, ()),
        # 128 x 128
        LinearCase(256, 128, 128, 2, 0, nb), LinearCase(385, 256, 160, 2, 0, nb), LinearCase(1027, 128, 128, 2, 3, nb),
    ]
    wide = [
        # 256 x 128: whole tiles; a ragged last tile; 5 tail rows and a half-empty last 256-row tile
        LinearCase(64 * cus, 512, 128, 3, 0, ()), LinearCase(64 * cus - 100, 512, 128, 3, 0, ()),
        LinearCase(64 * cus - 123, 512, 160, 3, 5, ()),
        # 256 x 256
        LinearCase(128 * cus, 512, 128, 4, 0, ()), LinearCase(128 * cus - 100, 512, 128, 4, 0, ()),
        LinearCase(128 * cus - 125, 512, 160, 4, 3, ()),
        # the same rows on the narrower tiles: bit-identical tile rows
        LinearCase(128 * cus, 512, 128, 3, 0, (("ISI_GEMM_NO_WIDE", 2),)), LinearCase(128 * cus, 512, 128, 2, 0, (("ISI_GEMM_NO_WIDE", 1),)),
    ]
    return small, wide


def linear_epilogue_args(which, M, N, ldo, bias, res, gate, seed=LINEAR_SEEDS[0], keep=None):
    """(bias, res, relu, gate, gate_scale, keep, p) of one of LINEAR_EPILOGUES: the arguments of linear_spec behind x and W.
    The mask is that of an output of row stride ldo (`keep`: a mask the caller computed already)."""
    p = LINEAR_DROP_P
    gs = 1.0 / (1.0 - p)
    mask = lambda: dropout_keep_mask(seed, M, N, ldo, p) if keep is None else keep
    return {"bias": lambda: (bias, None, False, None, 1.0, None, 0.0),
            "bias+res+relu": lambda: (bias, res, True, None, 1.0, None, 0.0),
            "gate": lambda: (bias, None, False, gate, gs, None, 0.0),
            "relu+dropout": lambda: (bias, None, True, None, 1.0, mask(), p),
            "all": lambda: (bias, res, True, gate, gs, mask(), p)}[which]()


LinearRefs = collections.namedtuple("LinearRefs", "x W bias res gate prod64 prod32 model")
_linear_refs_cache = {}


def linear_refs(M, N, K, device="cpu"):
    """The data of a shape (linear_case_data), its float64 and float32 products and the two modes' three-term models, on
    `device` (uncached; the wide shapes of the GPU test: torch's own matmuls there, 0.5 GB of references each)."""
    x, W, bias, res, gate = (t.to(device) for t in linear_case_data(M, N, K))
    model = {m: linear_split_model(x, W, m) for m in ("bf16", "f16")}
    return LinearRefs(x, W, bias, res, gate, x.double() @ W.double().t(), x @ W.t(), model)


def linear_case_refs(M, N, K):
    """linear_refs on the CPU, computed once per process and left unchanged: every shape below 1 M outputs."""
    if (M, N, K) not in _linear_refs_cache:
        _linear_refs_cache[(M, N, K)] = linear_refs(M, N, K)
    return _linear_refs_cache[(M, N, K)]


# Float64 specification of the fused quantize_conv + codebook search (vq_conv1x1_nearest_kernel of csrc/vq_nearest.hip, through
# isi_vq_conv1x1_nearest_f32 / isi_vq_conv1x1_nearest_tape_f32), its float32 yardstick, seeded case data that is free of
# near-ties by construction, and the comparisons of tests/test_vq_fused_gpu.py -- tests/test_vq_fused_host.py shows, without
# a GPU, what they reject.  Activations [N, C] channels-last (N = B H W pixels), W [64, C0 + C1], embed [D = 64, K].
VQ_FUSED_D = 64
VQ_FUSED_TILE = 256            # VQ_VEC_PER_BLOCK_ITER: pixels of one workgroup pass (8 waves of 32)
VQ_FUSED_GRID = 256            # vq_grid's cap: beyond 256 tiles a workgroup runs its tile loop again
VQ_FUSED_MIN_GAP = 1e-4        # ten times quantizer_large.npz's: z is computed here and carries the convolution's rounding
VQ_FUSED_ACT_LIMIT = 16384.0   # range of the pair format (include/isi_hip.h, ISI_CONV_F16X3): beyond it a pixel is loud
VQ_FUSED_SSE_RTOL = 1e-5       # tolerance of `diff` throughout tests/test_hip_parity.py
VqFusedSpec = collections.namedtuple("VqFusedSpec", "z idx q counts sse sse_rows diff perplexity")
VqFusedCase = collections.namedtuple("VqFusedCase", "C0 C1 K B H W strided")


def _vq_fused_top2(z, e):
    """(two smallest distances [n, 2], their codes [n, 2]) of d[n, k] = sum_d (z[n, d] - e[k, d])^2, written out as a difference
    (no cancelling three-term formula) in the dtype of z, in blocks of pixels.  A smaller distance first, the lower code first
    on exact equality.  One code only: the second distance is +inf."""
    n, K = z.shape[0], e.shape[0]
    step = max(1, 2 ** 22 // (K * z.shape[1]))
    best, code = [], []
    for lo in range(0, n, step):
        d = (z[lo:lo + step, None, :] - e[None, :, :]).pow(2).sum(dim=-1)
        if K == 1:
            d = torch.cat([d, torch.full_like(d, float("inf"))], dim=1)
        # (sorting by (distance, code): a stable sort of the distances keeps the lower code in front of its equals)
        ds, order = torch.sort(d, dim=1, stable=True)
        best.append(ds[:, :2])
        code.append(order[:, :2])
    return torch.cat(best), torch.cat(code)


def _vq_fused_eval(a0, a1, W, bias, embed, dtype):
    a = torch.as_tensor(a0).detach().cpu() if a1 is None else torch.cat([torch.as_tensor(a0).detach().cpu(), torch.as_tensor(a1).detach().cpu()], dim=1)
    W, embed = torch.as_tensor(W).detach().cpu(), torch.as_tensor(embed).detach().cpu()
    N, (D, K) = a.shape[0], embed.shape
    lost = ~torch.isfinite(a).all(dim=1) | (a.abs() >= VQ_FUSED_ACT_LIMIT).any(dim=1)
    if not bool(torch.isfinite(embed).all()):
        lost[:] = True
    z = torch.where(lost[:, None], torch.zeros_like(a), a).to(dtype) @ W.to(dtype).t()
    if bias is not None:
        z = z + torch.as_tensor(bias).detach().cpu().to(dtype)
    return _vq_search_eval(z, embed, lost, dtype)


def _vq_search_eval(z, embed, lost, dtype):
    """The search half of both specifications: VqFusedSpec of vectors z [N, D] (already of `dtype`) on embed [D, K]; `lost`
    [N] bool are the vectors the route gives up before it searches.  A code with a non-finite component takes no part (its
    distance is never below +inf) and the other codes rank as if it were absent; a vector left without a finite distance is
    lost as well.  Lost vectors: idx -1, q and z NaN, not counted, sse NaN."""
    N, (D, K) = z.shape[0], embed.shape
    e = embed.to(dtype).t().contiguous()
    absent = ~torch.isfinite(e).all(dim=1)
    if bool(absent.any()):
        e_rank = e.clone()
        e_rank[absent] = float("inf")                       # (inf - z)^2 = inf: behind every finite distance
        lost = lost | ~torch.isfinite(z).all(dim=1)
        if bool(absent.all()):
            lost = torch.ones_like(lost)
    else:
        e_rank = e
    live = ~lost
    idx = torch.full((N,), -1, dtype=torch.int64)
    q = torch.full((N, D), float("nan"), dtype=dtype)
    sse_rows = torch.full((N,), float("nan"), dtype=dtype)
    if bool(live.any()):
        idx[live] = _vq_fused_top2(z[live], e_rank)[1][:, 0]
        q[live] = e[idx[live]]
        sse_rows[live] = (q[live] - z[live]).pow(2).sum(dim=1)
    z = z.clone()
    z[lost] = float("nan")
    counts = torch.bincount(idx[live], minlength=K)
    sse = sse_rows.sum()
    diff, perplexity = vq_finalize_spec(sse.reshape(1), counts, N, D)
    return VqFusedSpec(z, idx, q, counts, sse, sse_rows, diff, perplexity)


def vq_fused_spec(a0, a1, W, bias, embed):
    """VqFusedSpec of the fused launch, everything float64: z = cat(a0, a1) W^T + bias; d = |z - e_k|^2 as a difference;
    idx = argmin, the lowest index on exact equality; q = e_idx; counts = bincount(idx, K); sse = sum (e_idx - z)^2 (sse_rows:
    per pixel); diff and perplexity through vq_finalize_spec.  A pixel with a non-finite activation, or one beyond the pair
    format's range (|a| >= 16384), has idx = -1, q = NaN (z likewise), is not counted and makes sse NaN; so does every pixel
    when a code is not finite (include/isi_hip.h, "quantization")."""
    return _vq_fused_eval(a0, a1, W, bias, embed, torch.float64)


def vq_fused_f32(a0, a1, W, bias, embed):
    """The same in float32 torch: the yardstick of z, and what the host tests apply their simulated defects to."""
    return _vq_fused_eval(a0, a1, W, bias, embed, torch.float32)


def vq_fused_split_z(a0, a1, W, bias):
    """Float64 evaluation of the three split-f16 terms the kernel keeps of the 1x1 convolution (linear_split_model, "f16"), plus
    the bias: the other half of the yardstick of z."""
    a = a0 if a1 is None else torch.cat([a0, a1], dim=1)
    return linear_split_model(a, W, "f16") + (0.0 if bias is None else _f64(bias))


def vq_fused_gaps(z, embed, alias=None):
    """Per pixel, the float64 gap between the best and the second-best code, normalised by |z|^2 + |e_best|^2 (the metric of
    oracle.near_tie_free_vectors).  `alias` [K] (code -> the lowest index holding the same vector): duplicates of a code take no
    part, so a pixel that ties between duplicates is measured against every OTHER code."""
    z, e = _f64(z), _f64(embed).t().contiguous()
    if alias is not None:
        e = e.clone()
        e[alias != torch.arange(e.shape[0])] = float("inf")      # (inf - z)^2 = inf: never among the two best
    best, code = _vq_fused_top2(z, e)
    return (best[:, 1] - best[:, 0]) / (z.pow(2).sum(dim=1) + e[code[:, 0]].pow(2).sum(dim=1))


def _vq_fused_draw(n, C, gen):
    """Rectified Gaussian activations, as the models' are, rounded so that the pair format holds them exactly."""
    return pair_round_f16(torch.randn(n, C, generator=gen).clamp(min=0.0))


def vq_fused_settle(a, W, bias, embed, gen, alias=None, frozen=None, min_gap=VQ_FUSED_MIN_GAP):
    """Redraws every pixel (row of a [N, C]) whose gap is below min_gap until none remains; `frozen` [N] bool: pixels a test
    placed by hand, never redrawn (the caller checks their gaps).  Returns the settled copy."""
    a = a.clone()
    Wd, bd = _f64(W), _f64(bias)
    rows = torch.arange(a.shape[0]) if frozen is None else (~frozen).nonzero().reshape(-1)
    for _ in range(64):
        if rows.numel() == 0:
            return a
        low = vq_fused_gaps(a[rows].double() @ Wd.t() + bd, embed, alias) < min_gap
        rows = rows[low]
        a[rows] = _vq_fused_draw(rows.numel(), a.shape[1], gen)
    raise AssertionError("vq_fused_settle: near-ties remain after 64 redraws")


VQ_FUSED_DUP_SOURCES = (3, 70, 141)           # where the three most-used codes are moved to, and per source its two copies:
VQ_FUSED_DUP_COPIES = ((7, 68), (74, 167), (145, 270))   # the other lane half of the same 32-row tile (bit 2 of the row), another tile


def vq_fused_duplicate_codes(a, W, bias, embed):
    """(embed', alias): the three most-used codes of the data moved to VQ_FUSED_DUP_SOURCES and copied to VQ_FUSED_DUP_COPIES,
    all at higher indices; alias as vq_fused_gaps takes it."""
    K = embed.shape[1]
    z = a.double() @ _f64(W).t() + _f64(bias)
    idx = _vq_fused_top2(z, _f64(embed).t().contiguous())[1][:, 0]
    top = torch.bincount(idx, minlength=K).argsort(descending=True, stable=True)[:3].tolist()
    embed = embed.clone()
    for src, k in zip(VQ_FUSED_DUP_SOURCES, top):
        cur = k
        for s2, k2 in zip(VQ_FUSED_DUP_SOURCES, top):     # (an earlier swap may have moved this code)
            if s2 == src:
                break
            cur = k2 if cur == s2 else (s2 if cur == k2 else cur)
        tmp = embed[:, src].clone()
        embed[:, src] = embed[:, cur]
        embed[:, cur] = tmp
    alias = torch.arange(K)
    for src, copies in zip(VQ_FUSED_DUP_SOURCES, VQ_FUSED_DUP_COPIES):
        for c in copies:
            assert c > src and c < K
            embed[:, c] = embed[:, src]
            alias[c] = src
    return embed, alias


def vq_fused_case_seed(case):
    return ((case.C0 * 263 + case.C1) * 4099 + case.K) * 70001 + case.B * case.H * case.W


def vq_fused_case_data(case, seed=None, dups=False, W=None, bias=None):
    """(a0 [N, C0], a1 [N, C1] or None, W [64, C], bias [64], embed [64, K], alias or None) float32 on the CPU, seeded.  The
    activations are rectified and rounded by pair_round_f16; W ~ N(0, 1 / C), bias ~ 0.1 N(0, 1); the codebook is K of the spec's
    own z vectors (of max(N, 2 K) drawn pixels, the first N being the data: at N < 2 K some pixels have a code of their own and
    the others do not, as at N >> K) plus 0.05 N(0, 1) jitter, so the codes lie where the data is; then every pixel with a gap (vq_fused_gaps) below VQ_FUSED_MIN_GAP is redrawn until none remains.  Measured for
    C in {32, 192, 256}, K = 512, N = 66 603: 0.3 % of the draws fall below 1e-4 and a float32 evaluation of the whole formula
    flips an index only at gaps of about 1e-7 -- three decades of room, so the indices of a correct kernel equal the spec's,
    all of them.  `dups`: vq_fused_duplicate_codes first; the pixels that tie between duplicates are exempt from the gap
    against their duplicates, and only against those.  `W`, `bias`: given ones in place of the drawn."""
    C, N, K = case.C0 + case.C1, case.B * case.H * case.W, case.K
    gen = torch.Generator().manual_seed(vq_fused_case_seed(case) if seed is None else seed)
    pool = _vq_fused_draw(max(N, 2 * K), C, gen)
    Wr = torch.randn(VQ_FUSED_D, C, generator=gen) / C ** 0.5
    br = 0.1 * torch.randn(VQ_FUSED_D, generator=gen)
    W, bias = Wr if W is None else W, br if bias is None else bias
    z = pool.double() @ W.double().t() + bias.double()
    pick = torch.randperm(pool.shape[0], generator=gen)[:K]
    embed = (z[pick] + 0.05 * torch.randn(K, VQ_FUSED_D, generator=gen).double()).float().t().contiguous()
    a, alias = pool[:N], None
    if dups:
        embed, alias = vq_fused_duplicate_codes(a, W, bias, embed)
    a = vq_fused_settle(a, W, bias, embed, gen, alias)
    return a[:, :case.C0].contiguous(), (a[:, case.C0:].contiguous() if case.C1 else None), W, bias, embed, alias


VQ_FUSED_FAR_PIXELS = {5: 200, 11: 320}       # hand-placed pixel -> the far code that is its nearest


def vq_fused_far_case_data(case):
    """The constructions of test_codebook_beyond_f16_range for the fused launch (C0 + C1 >= 96, K = 512): W is an identity block
    on channels 32 .. 95 (both sources at (64, 128)) and zero elsewhere, the bias zero, so z is those 64 activations.  40 dead
    codes scaled by 3e4; one code at 1e5 times its neighbour; pixel 5, whose nearest code (200) has a component of 70; a far
    code of moderate norm (320: 200 in one component) with pixel 11 next to it, which no certificate covers -- the fp32 scan
    decides.  Every other pixel is settled against the edited codebook.  Returns vq_fused_case_data's tuple."""
    C = case.C0 + case.C1
    assert C >= 96 and case.K == 512
    W = torch.zeros(VQ_FUSED_D, C)
    W[:, 32:96] = torch.eye(VQ_FUSED_D)
    bias = torch.zeros(VQ_FUSED_D)
    a0, a1, _, _, embed, _ = vq_fused_case_data(case, seed=vq_fused_case_seed(case) + 1, W=W, bias=bias)
    a = a0 if a1 is None else torch.cat([a0, a1], dim=1)
    a[5], a[11] = 0.0, 0.0
    a[5, 32 + 7], a[11, 32 + 3] = 70.0, 198.0
    embed[:, 300:340] *= 3.0e4
    embed[:, 17] = embed[:, 16] * 1.0e5
    embed[:, 200] = a[5, 32:96]
    embed[:, 320] = 0.0
    embed[3, 320] = 200.0
    frozen = torch.zeros(a.shape[0], dtype=torch.bool)
    frozen[list(VQ_FUSED_FAR_PIXELS)] = True
    a = vq_fused_settle(a, W, bias, embed, torch.Generator().manual_seed(vq_fused_case_seed(case) + 2), frozen=frozen)
    return a[:, :case.C0].contiguous(), (a[:, case.C0:].contiguous() if case.C1 else None), W, bias, embed, None


VqFusedRefs = collections.namedtuple("VqFusedRefs", "a0 a1 W bias embed alias spec f32 z_yard")

def vq_fused_refs(a0, a1, W, bias, embed, alias=None):
    """Spec, float32 evaluation and the yardstick of z -- per element the worse of the float32 evaluation and the three-term
    split-f16 model -- of given operands."""
    spec, f32 = vq_fused_spec(a0, a1, W, bias, embed), vq_fused_f32(a0, a1, W, bias, embed)
    live = spec.idx >= 0
    yard = torch.full_like(spec.z, float("nan"))
    if bool(live.any()):
        a1l = None if a1 is None else a1[live]
        yard[live] = larger_error(f32.z[live], vq_fused_split_z(a0[live], a1l, W, bias), spec.z[live])
    return VqFusedRefs(a0, a1, W, bias, embed, alias, spec, f32, yard)


@functools.lru_cache(maxsize=None)
def vq_fused_case_refs(case, dups=False):
    """vq_fused_refs of vq_fused_case_data, computed once per process and left unchanged."""
    return vq_fused_refs(*vq_fused_case_data(case, dups=dups))


def _vfc(C0, C1, K, shape, strided=False):
    return VqFusedCase(C0, C1, K, *shape, strided)


# (B, H, W) per pixel count: 257 and 31 are prime; 255, 256 and 66 603 decompose in all three dimensions of pixel_offsets
VQ_FUSED_SHAPES = {1: (1, 1, 1), 31: (1, 31, 1), 33: (3, 1, 11), 255: (3, 5, 17), 256: (4, 8, 8), 257: (1, 1, 257),
                   66603: (3, 149, 149)}
# channel routes (C0, C1) -> the chunk-count template NCH: 32 and 96 leave a dead chunk, (96, 160) starts the second source
# on an odd chunk
VQ_FUSED_ROUTES = {(32, 0): 2, (64, 0): 2, (96, 0): 4, (128, 0): 4, (256, 0): 8, (32, 32): 2, (64, 128): 6, (96, 160): 8}
VQ_FUSED_ROUTE_CASES = [_vfc(c0, c1, 512, VQ_FUSED_SHAPES[257]) for c0, c1 in VQ_FUSED_ROUTES]
# pixel counts: below one wave's 32 vectors, one past it, around one tile, and 260 full tiles + 43 vectors (workgroups 0..4 run
# a second pass, the last tile is ragged; K = 64 there: its float64 reference takes about a second)
VQ_FUSED_PIXEL_CASES = ([_vfc(64, 128, 512, VQ_FUSED_SHAPES[n]) for n in (1, 31, 33, 255, 256, 257)]
                        + [_vfc(32, 0, 64, VQ_FUSED_SHAPES[n]) for n in (1, 31, 33, 255, 256, 257, 66603)])
VQ_FUSED_K_SIZES = (16, 40, 500, 512)         # ... and K_max, which the tests ask isi_vq_conv1x1_fusable for
# cropped channel slices of wider maps (VQ_FUSED_PARENTS); 255 = 3 x 5 x 17 moves through every stride at a small size
VQ_FUSED_STRIDED_CASES = [_vfc(64, 128, 512, (1, 257, 1), True), _vfc(64, 128, 512, VQ_FUSED_SHAPES[255], True),
                          _vfc(64, 128, 64, VQ_FUSED_SHAPES[66603], True)]
# per source: (channels the parent map has beyond the slice, first channel of the slice, rows above, below, columns left, right
# of the crop):
# different parents, different strides, and a nonzero pointer offset for both
VQ_FUSED_PARENTS = ((64, 32, 1, 1, 2, 1), (96, 64, 2, 1, 1, 0))


def vq_fused_k_cases(k_max):
    return [_vfc(64, 0, K, VQ_FUSED_SHAPES[257]) for K in VQ_FUSED_K_SIZES + (k_max,)]


def vq_fused_k_max(L):
    """The largest K isi_vq_conv1x1_fusable(64, 0, 64, K) accepts (the library's answer; it is monotone in K)."""
    ks = [K for K in range(1, 4097) if L.isi_vq_conv1x1_fusable(64, 0, VQ_FUSED_D, K) == 1]
    assert ks and ks == list(range(1, ks[-1] + 1)), "isi_vq_conv1x1_fusable is not monotone in K"
    return ks[-1]


def vq_fused_case_id(c):
    return f"C{c.C0}+{c.C1}-K{c.K}-{c.B}x{c.H}x{c.W}" + ("-strided" if c.strided else "")


def vq_num_partials(N):
    """isi_vq_num_partials: one partial per workgroup of vq_grid."""
    return min(VQ_FUSED_GRID, max(1, -(-N // VQ_FUSED_TILE)))


def vq_fused_partials(sse_rows):
    """sse_part as the kernel's workgroups own it: workgroup g sums the tiles g, g + 256, ... of 256 pixels."""
    N = sse_rows.shape[0]
    n_part = vq_num_partials(N)
    tile = torch.arange(N) // VQ_FUSED_TILE
    return torch.zeros(n_part, dtype=sse_rows.dtype).index_add_(0, tile % n_part, sse_rows)


def pair_encode_host(x):
    """The pair format of csrc/split_f16.h on the CPU: per group of 8 consecutive floats {hi[8] | lo[8]}, the f16 pieces of
    4 x, in a float32-typed tensor of x's shape (its bits are what matters)."""
    xs = x.float().contiguous() * 4.0
    hi = xs.half()
    lo = (xs - hi.float()).half()
    g = torch.stack([hi.reshape(-1, 8), lo.reshape(-1, 8)], dim=1)
    return g.reshape(-1).view(torch.float32).reshape(x.shape)


def pair_decode_host(p):
    """(hi + lo) / 4 of every element of a pair-format tensor."""
    h = p.detach().cpu().contiguous().reshape(-1).view(torch.float16).reshape(-1, 2, 8).float()
    return ((h[:, 0] + h[:, 1]) / 4.0).reshape(p.shape)


# The comparisons.  Each takes a launch's output as a CPU tensor and raises AssertionError with `what` in front.
def vq_fused_hold_idx(idx, spec, what):
    """Every index equals the spec's: the data has no near-tie, so the cap on differing indices is zero."""
    idx = torch.as_tensor(idx).cpu().reshape(-1)
    assert idx.dtype == torch.int64 and idx.shape == spec.idx.shape, f"{what}: idx {idx.dtype} {tuple(idx.shape)}"
    bad = (idx != spec.idx).nonzero().reshape(-1)
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {idx.numel()} indices differ from the float64 spec's, first at pixel "
                              f"{int(bad[0])}: {int(idx[bad[0]])} against {int(spec.idx[bad[0]])}")


def vq_fused_hold_counts(counts, spec, what):
    counts = torch.as_tensor(counts).cpu().reshape(-1).long()
    assert counts.shape == spec.counts.shape and torch.equal(counts, spec.counts), \
        f"{what}: counts differ from the spec's histogram (sum {int(counts.sum())} against {int(spec.counts.sum())})"


def vq_fused_hold_z(z, refs, what, margin=ROW_OPS_MARGIN):
    """z of the pixels the spec keeps through compare_rows against refs.z_yard; returns the RowCheck."""
    live = refs.spec.idx >= 0
    return compare_rows(torch.as_tensor(z).cpu()[live], refs.spec.z[live], refs.z_yard[live], f"{what} z", margin)


def vq_fused_hold_q(q, refs, what):
    """q = z + (e_idx - z) in float32: every element within one float32 ulp of max(|z|, |e|), 2^-23 of it, from e_idx; a pixel
    without a code is NaN throughout."""
    q, spec = torch.as_tensor(q).cpu(), refs.spec
    live = spec.idx >= 0
    assert q.shape == spec.q.shape and bool(torch.isnan(q[~live]).all()), f"{what}: q of a pixel without a code is not NaN"
    e, z = spec.q[live], spec.z[live]
    err = (q[live].double() - e).abs()
    assert bool(torch.isfinite(q[live]).all()), f"{what}: q is not finite"
    over = err - 2.0 ** -23 * torch.maximum(z.abs(), e.abs())
    assert float(over.max() if over.numel() else 0.0) <= 0.0, \
        f"{what}: q is further than one float32 ulp of max(|z|, |e|) from e_idx (largest error {float(err.max()):.3e})"


def vq_fused_hold_q_pair(q_pair, q, refs, what):
    """pair_decode(q_pair) within 2^-23 max|q| of q; NaN pieces where q is NaN."""
    dec, q = pair_decode_host(torch.as_tensor(q_pair).cpu()), torch.as_tensor(q).cpu()
    live = refs.spec.idx >= 0
    assert bool(torch.isnan(dec[~live]).all()), f"{what}: q_pair of a pixel without a code does not decode to NaN"
    if bool(live.any()):
        err, scale = float((dec[live] - q[live]).abs().max()), float(q[live].abs().max())
        assert math.isfinite(err) and err <= 2.0 ** -23 * scale, f"{what}: pair_decode(q_pair) is {err:.3e} from q (max|q| {scale:.3e})"


def vq_fused_hold_sse(sse_part, spec, what):
    """Every partial written (the buffer starts as NaN), their float64 sum within 1e-5 of the spec's; NaN where the spec's is."""
    sse_part = torch.as_tensor(sse_part).cpu().reshape(-1)
    assert sse_part.numel() == vq_num_partials(spec.idx.numel()), f"{what}: {sse_part.numel()} partials"
    total = float(sse_part.double().sum())
    if math.isnan(float(spec.sse)):
        assert math.isnan(total), f"{what}: the squared error of a launch with a lost pixel is {total}, not NaN"
        return
    assert not bool(torch.isnan(sse_part).any()), f"{what}: {int(torch.isnan(sse_part).sum())} partials were not written"
    assert abs(total - float(spec.sse)) <= VQ_FUSED_SSE_RTOL * float(spec.sse), \
        f"{what}: summed squared error {total!r} against the spec's {float(spec.sse)!r}"


# ---------------------------------------------------------------------------------------------------------------------
# The stand-alone codebook searches (vq_nearest_kernel<D> and vq_nearest_f16x3_kernel of csrc/vq_nearest.hip with the shared
# distance stage of csrc/vq_dist.h, through isi_vq_nearest_f32 / isi_vq_nearest_flags_f32) and pack_codebook_kernel of
# csrc/pack.hip: the search half of the fused specification applied to a GIVEN z, the loss rules of each route, K_max from
# the two LDS formulas, seeded case data free of near-ties, and the case table of tests/test_vq_search_gpu.py --
# tests/test_vq_search_host.py shows, without a GPU, what it relies on.  z [N, D], embed [D, K].
VQ_EXACT, VQ_F16X3 = "exact", "f16x3"
VQ_SEARCH_DIMS = (8, 16, 32, 64)
VQ_SEARCH_ROUTES = tuple((VQ_EXACT, D) for D in VQ_SEARCH_DIMS) + ((VQ_F16X3, 64),)
VQ_LDS_BUDGET = 150 * 1024     # kVqLdsBudget
VQ_SEARCH_WAVES = 8            # ISI_VQ_WAVES
VQ_SEARCH_SECOND_PASS_N = VQ_FUSED_GRID * VQ_FUSED_TILE + 257     # workgroups 0 and 1 run a second pass, the second one ragged
VqSearchCase = collections.namedtuple("VqSearchCase", "route D K N kind")
VqSearchRefs = collections.namedtuple("VqSearchRefs", "z embed alias frozen spec f32")


def vq_search_lost(z, embed, route):
    """[N] bool, the vectors a route gives up (include/isi_hip.h, "quantization").  Exact: a non-finite component.  f16x3:
    also a component beyond the pieces' range (|z| >= 16384), and every vector when a code is not finite."""
    z, embed = torch.as_tensor(z).detach().cpu(), torch.as_tensor(embed).detach().cpu()
    lost = ~torch.isfinite(z).all(dim=1)
    if route == VQ_F16X3:
        lost = lost | (z.abs() >= VQ_FUSED_ACT_LIMIT).any(dim=1)
        if not bool(torch.isfinite(embed).all()):
            lost = torch.ones_like(lost)
    else:
        assert route == VQ_EXACT, route
    return lost


def _vq_search(z, embed, route, dtype):
    z, embed = torch.as_tensor(z).detach().cpu(), torch.as_tensor(embed).detach().cpu()
    return _vq_search_eval(z.to(dtype), embed, vq_search_lost(z, embed, route), dtype)


def vq_search_spec(z, embed, route=VQ_EXACT):
    """VqFusedSpec of a stand-alone search, everything float64: the search half of vq_fused_spec (_vq_search_eval) on the
    given z, with the route's loss rules (vq_search_lost).  On the exact route a non-finite code never wins and the other
    codes rank as if it were absent."""
    return _vq_search(z, embed, route, torch.float64)


def vq_search_f32(z, embed, route=VQ_EXACT):
    """The same in float32 torch: what the host tests apply their simulated defects to."""
    return _vq_search(z, embed, route, torch.float32)


def vq_search_lds_bytes(D, Kp, split):
    """vq_exact_lds_bytes<D> (csrc/vq_dist.h) or, `split`, vq_planes_lds_bytes (csrc/vq_nearest.hip) of Kp padded codes."""
    if split:
        assert D == 64
        return Kp * 64 * 2 * 2 + (2 * Kp + VQ_SEARCH_WAVES + 1 + Kp // 32 + 3) * 4
    return (Kp * (D + 4) + 2 * Kp + VQ_SEARCH_WAVES) * 4


def vq_search_k_max(D, split=False):
    """The largest K whose LDS image (K rounded up to the 32-code tile) stays within the 150 KiB budget: 2720, 1728, 992 and
    544 for the exact route at D = 8, 16, 32, 64; 576 for the split-f16 route.  The GPU test holds the library to it."""
    Kp = 32
    assert vq_search_lds_bytes(D, Kp, split) <= VQ_LDS_BUDGET
    while vq_search_lds_bytes(D, Kp + 32, split) <= VQ_LDS_BUDGET:
        Kp += 32
    return Kp


def vq_search_gaps(z, embed, alias=None):
    """vq_fused_gaps of given vectors, for data with non-finite entries: a non-finite code takes no part (as in the spec), a
    non-finite vector has the gap NaN."""
    z, embed = _f64(z), _f64(embed).clone()
    embed[:, ~torch.isfinite(embed).all(dim=0)] = float("inf")
    bad = ~torch.isfinite(z).all(dim=1)
    gaps = vq_fused_gaps(torch.where(bad[:, None], torch.zeros_like(z), z), embed, alias)
    gaps[bad] = float("nan")
    return gaps


def _vq_search_draw(n, D, gen):
    return 0.8 * torch.randn(n, D, generator=gen)


def vq_search_settle(z, embed, gen, alias=None, frozen=None, min_gap=VQ_FUSED_MIN_GAP):
    """Redraws every vector whose gap (vq_search_gaps) is below min_gap until none remains; `frozen` [N] bool: rows a case
    placed by hand, never redrawn (tests/test_vq_search_host.py asserts their gaps).  Returns the settled copy.
    Why 1e-4 suffices on the split-f16 route as well: its ranking truncates 2^-19 of a distance and adds a margin of 2^-20
    |z|^2, a distance is at most 2 (|z|^2 + |e|^2), so the ranking moves a distance by less than 2^-18 + 2^-20 = 4.8e-6 of
    |z|^2 + |e|^2 -- a gap of 1e-4 of that keeps the true best code among the two candidates, and strictly first in the
    fp32 decision (rounding ~2^-22), with more than twenty times to spare.  No index may differ."""
    z = z.clone()
    rows = torch.arange(z.shape[0]) if frozen is None else (~frozen).nonzero().reshape(-1)
    for _ in range(64):
        if rows.numel() == 0:
            return z
        rows = rows[vq_search_gaps(z[rows], embed, alias) < min_gap]
        z[rows] = _vq_search_draw(rows.numel(), z.shape[1], gen)
    raise AssertionError("vq_search_settle: near-ties remain after 64 redraws")


VQ_SEARCH_KINDS = ("plain", "edges", "dups", "lost", "badcode", "far_certified", "far_scan", "far_pad", "far_all")
VQ_SEARCH_EDGE_ROWS = {"code": 2, "zero": 9, "tiny": 20}      # a row equal to code K // 2, the zero vector, a row of norm 1e-3
VQ_SEARCH_DUP_ROWS = (1, 34, 256)                             # rows laid exactly on the duplicated codes (256: the ragged tile)
VQ_SEARCH_LOST_ROWS = {3: float("nan"), 40: float("inf"), 599: float("-inf")}   # row -> the value of one of its components
VQ_SEARCH_LOUD_ROW, VQ_SEARCH_LOUD_CODE = 70, 17              # a finite row with a component of 3e4, and its nearest code
VQ_SEARCH_BAD_CODES = {10: float("inf"), 37: float("nan"), -1: float("-inf")}   # code -> one component (-1: the last code)
VQ_SEARCH_FAR_ROWS = {"far_scan": VQ_FUSED_FAR_PIXELS, "far_pad": {11: 98}}     # hand-placed row -> the far code nearest to it


def vq_search_dup_layout(K):
    """(sources, copies per source): VQ_FUSED_DUP_* where K allows, else an analogue of the same structure -- per source a
    copy in the other lane half of the same 32-row tile (bit 2 of the row differs) and one in another tile, both at higher
    indices."""
    if K > max(max(c) for c in VQ_FUSED_DUP_COPIES):
        return VQ_FUSED_DUP_SOURCES, VQ_FUSED_DUP_COPIES
    if K >= 96:
        return (3, 40), ((7, 68), (44, 75))
    assert K >= 64, K
    return (3, 9), ((7, 35), (13, 41))


def vq_search_case_seed(c):
    """(Not a function of the route: the two routes of D = 64 search the same data.)"""
    return ((c.D * 4099 + c.K) * 70001 + c.N) * 16 + VQ_SEARCH_KINDS.index(c.kind)


def vq_search_case_data(c):
    """(z [N, D], embed [D, K], alias or None, frozen [N] bool) float32 on the CPU, seeded: codes ~ N(0, 0.7^2), vectors
    ~ N(0, 0.8^2) (at most 0.3 % of such rows have a gap below 1e-4 at any (D, K) of the table), the kind's hand-placed rows
    and codes, then every other row settled (vq_search_settle).
      plain          nothing placed
      edges          a row equal to a code bit for bit, the zero vector, a row of norm 1e-3 (the LDS image's padding rows are
                     zero vectors: with anything but a losing |e|^2 they would win the last two); the code of the smallest
                     norm is shrunk by 0.9 so that the origin has no near-tie
      dups           vq_search_dup_layout; VQ_SEARCH_DUP_ROWS lie exactly on the duplicated codes
      lost           VQ_SEARCH_LOST_ROWS hold NaN, +Inf, -Inf; row VQ_SEARCH_LOUD_ROW is finite with a component of 3e4, beyond
                     the split-f16 route's range -- the exact route answers it: code VQ_SEARCH_LOUD_CODE has 6.0 there, which
                     puts it 6e4 (6 - 1.8) / 9e8 = 2.8e-4 of |z|^2 in front of every other code
      badcode        VQ_SEARCH_BAD_CODES: three codes with a non-finite component, one of them in the padded last tile
      far_certified  ten codes scaled by 3e4: the certificate of vq_decide_f32 holds for every row
      far_scan       the constructions of vq_fused_far_case_data: 40 dead codes, a code at 1e5 times its neighbour, and the
                     two rows of VQ_FUSED_FAR_PIXELS, which the fp32 scan decides
      far_pad        a far code of moderate norm in the padded last tile (K = 100: code 98) with row 11 next to it, code 99 dead
      far_all        every code is far (scaled by 1e3): no candidate at all, the scan answers every row"""
    D, K, N, kind = c.D, c.K, c.N, c.kind
    gen = torch.Generator().manual_seed(vq_search_case_seed(c))
    embed = 0.7 * torch.randn(D, K, generator=gen)
    z = _vq_search_draw(N, D, gen)
    frozen, alias = torch.zeros(N, dtype=torch.bool), None

    def far_pair(row, code, comp=3):       # a far code of moderate norm and a row next to it
        embed[:, code] = 0.0
        embed[comp, code] = 200.0
        z[row] = 0.0
        z[row, comp] = 198.0
        frozen[row] = True

    if kind == "edges":
        assert N >= 33 and K >= 2
        embed[:, embed.pow(2).sum(dim=0).argmin()] *= 0.9
        v = torch.randn(D, generator=gen)
        z[VQ_SEARCH_EDGE_ROWS["code"]] = embed[:, K // 2]
        z[VQ_SEARCH_EDGE_ROWS["zero"]] = 0.0
        z[VQ_SEARCH_EDGE_ROWS["tiny"]] = 1e-3 * v / v.norm()
        frozen[list(VQ_SEARCH_EDGE_ROWS.values())] = True
    elif kind == "dups":
        sources, copies = vq_search_dup_layout(K)
        alias = torch.arange(K)
        for src, cs, row in zip(sources, copies, VQ_SEARCH_DUP_ROWS):
            for k in cs:
                assert src < k < K
                embed[:, k] = embed[:, src]
                alias[k] = src
            z[row] = embed[:, src]
            frozen[row] = True
    elif kind == "lost":
        assert N > max(VQ_SEARCH_LOST_ROWS) and K > VQ_SEARCH_LOUD_CODE and D >= 8
        embed[5, VQ_SEARCH_LOUD_CODE] = 6.0
        for comp, (row, value) in zip((1, D - 1, 0), VQ_SEARCH_LOST_ROWS.items()):
            z[row, comp] = value
            frozen[row] = True
        z[VQ_SEARCH_LOUD_ROW, 5] = 3.0e4
        frozen[VQ_SEARCH_LOUD_ROW] = True
    elif kind == "badcode":
        for comp, (code, value) in zip((2, 0, 1), VQ_SEARCH_BAD_CODES.items()):
            embed[comp, code] = value
    elif kind == "far_certified":
        embed[:, 130:140] *= 3.0e4
    elif kind == "far_scan":
        assert D == 64 and K == 512
        embed[:, 300:340] *= 3.0e4
        embed[:, 17] = embed[:, 16] * 1.0e5
        z[5] = 0.0
        z[5, 7] = 70.0
        embed[:, 200] = z[5]
        frozen[5] = True
        far_pair(11, 320)
    elif kind == "far_pad":
        assert D == 64 and K == 100
        far_pair(11, 98)
        embed[:, 99] *= 3.0e4
    elif kind == "far_all":
        embed *= 1.0e3
    else:
        assert kind == "plain", kind
    return vq_search_settle(z, embed, gen, alias, frozen), embed, alias, frozen


@functools.lru_cache(maxsize=None)
def vq_search_case_refs(c):
    """VqSearchRefs of a case -- its data, the float64 spec and the float32 evaluation on the case's route -- computed once
    per process and left unchanged."""
    z, embed, alias, frozen = vq_search_case_data(c)
    return VqSearchRefs(z, embed, alias, frozen, vq_search_spec(z, embed, c.route), vq_search_f32(z, embed, c.route))


def _vq_search_table():
    cases = []
    for route, D in VQ_SEARCH_ROUTES:
        split = route == VQ_F16X3
        # K: one code, one ragged tile, around one tile, 2 tiles (an even count), 3 tiles (odd), 4 tiles with a ragged last
        # one, 5 tiles, (f16x3: 545, beyond what the exact route accepts at D = 64,) and the route's K_max
        ks = (1, 5, 31, 32, 33, 64, 96, 100, 160) + ((545,) if split else ()) + (vq_search_k_max(D, split),)
        cases += [VqSearchCase(route, D, K, 257, "plain") for K in ks]
        cases += [VqSearchCase(route, D, 100, N, "plain") for N in (1, 31, 32, 33, 255, 256)]
        cases += [VqSearchCase(route, D, 100, 257, "edges"), VqSearchCase(route, D, 96, 257, "dups"),
                  VqSearchCase(route, D, 100, 600, "lost"), VqSearchCase(route, D, 100, 257, "badcode")]
        if D == 64:
            cases += [VqSearchCase(route, D, 64, 257, "dups"), VqSearchCase(route, D, 512, 257, "dups")]
    # the second grid-stride pass, one per route (their float64 specs take seconds on the CPU)
    cases += [VqSearchCase(VQ_EXACT, 8, 33, VQ_SEARCH_SECOND_PASS_N, "plain"), VqSearchCase(VQ_F16X3, 64, 96, VQ_SEARCH_SECOND_PASS_N, "plain")]
    cases += [VqSearchCase(VQ_F16X3, 64, 160, 257, "far_certified"), VqSearchCase(VQ_F16X3, 64, 512, 257, "far_scan"),
              VqSearchCase(VQ_F16X3, 64, 100, 257, "far_pad"), VqSearchCase(VQ_F16X3, 64, 5, 257, "far_all")]
    return cases


VQ_SEARCH_CASES = _vq_search_table()


def vq_search_case_id(c):
    return f"{c.route}-D{c.D}-K{c.K}-N{c.N}-{c.kind}"


def vq_search_coverage_gaps(cases):
    """What a case table lacks of the corners the stand-alone searches have (an empty list: nothing): per route and D tile
    counts 1 to 5 (3 and 5: the odd exit of the split-f16 tile pipeline and the prefetch behind an odd last tile), the
    route's K_max, a ragged last tile, vector counts on both sides of a wave's 32 and a workgroup's 256, every data kind
    the route has; per route a second grid-stride pass; on the split-f16 route 545 codes and the four far-code kinds."""
    lack = []
    for route, D in VQ_SEARCH_ROUTES:
        mine = [c for c in cases if (c.route, c.D) == (route, D)]
        name = f"{route} D={D}"
        tiles = {(c.K + 31) // 32 for c in mine}
        lack += [f"{name}: no codebook of {t} tiles" for t in (1, 2, 3, 4, 5) if t not in tiles]
        ks, ns = {c.K for c in mine}, {c.N for c in mine}
        if vq_search_k_max(D, route == VQ_F16X3) not in ks:
            lack.append(f"{name}: K_max is missing")
        if not any(K % 32 and K > 32 for K in ks):
            lack.append(f"{name}: no ragged last tile behind a full one")
        lack += [f"{name}: no launch of {n} vectors" for n in (1, 31, 32, 33, 255, 256, 257) if n not in ns]
        kinds = {c.kind for c in mine}
        lack += [f"{name}: no case of kind {k}" for k in ("plain", "edges", "dups", "lost", "badcode") if k not in kinds]
    for route in (VQ_EXACT, VQ_F16X3):
        if not any(c.route == route and -(-c.N // VQ_FUSED_TILE) > VQ_FUSED_GRID and c.N % VQ_FUSED_TILE for c in cases):
            lack.append(f"{route}: no second grid-stride pass with a ragged tile")
    split = [c for c in cases if c.route == VQ_F16X3]
    if not any(c.K > vq_search_k_max(64) for c in split):
        lack.append("f16x3: no codebook beyond the exact route's K_max")
    lack += [f"f16x3: no case of kind {k}" for k in ("far_certified", "far_scan", "far_pad", "far_all") if k not in {c.kind for c in split}]
    for c in cases:
        if c.kind in ("dups",) and c.N != 257 or c.kind == "edges" and c.N < 33 or c.kind == "lost" and c.N <= max(VQ_SEARCH_LOST_ROWS):
            lack.append(f"{vq_search_case_id(c)}: too few vectors for its hand-placed rows")
    return lack


def vq_pack_codebook_spec(embed):
    """(codes [K, D]: the transpose, bit for bit; e2 [K, 1] float64: |e_k|^2) of isi_pack_codebook_f32 on embed [D, K]."""
    e = torch.as_tensor(embed).detach().cpu()
    return e.t().contiguous(), _f64(e).pow(2).sum(dim=0).reshape(-1, 1)


def vq_pack_codebook_f32(embed, exchanged=False):
    """|e_k|^2 [K, 1] as a float32 sum over d in sequence, the yardstick of e2.  Mutant `exchanged`: element (d, k) read at
    d * D + k -- D and K exchanged in the index (K >= D keeps it inside the array)."""
    e = torch.as_tensor(embed).detach().cpu().float()
    D, K = e.shape
    if exchanged:
        assert K >= D
        e = e.reshape(-1)[(torch.arange(D)[:, None] * D + torch.arange(K)[None, :])]
    s = torch.zeros(K)
    for d in range(D):
        s = s + e[d] * e[d]
    return s.reshape(-1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# The stage kernels of the key/value-cached decoding loop (csrc/prior_decode.hip through isi_decode_stage_ex_f32 and
# isi_decode_single_source_f32): float64 specifications, their float32 evaluations (the yardsticks of compare_rows and
# what the host tests apply their mutants to), and the route table -- one case per route of the host plan `stage_kernel()`
# and of the launchers' template instantiations.  tests/test_decode_stage_host.py holds the specs to float64 torch and shows
# that every mutant falls outside the bound; tests/test_decode_stage_gpu.py holds the kernels to the specs;
# tests/decode_plan_tracer.cpp runs the same cases (`stagex/...`, kStageExCases) through the host plan without a GPU.
DECODE_STAGE_POSITIONS = 3       # slots of every position-addressed array of a case (x, res, the k|v cache)
DECODE_STAGE_P = 1               # the position (or step of row_pos) a case addresses, by value or in the device counter
DECODE_STAGE_ROW_INVARIANCE = 4e-6   # a row of a batch against the row alone, GEMV families (tests/test_prior_gpu.py's allowance)
STAGE_ONE_ROW, STAGE_TILES, STAGE_ROWS_IN_REGISTERS, STAGE_GROUPS_OF_8, STAGE_REFUSED = range(5)
STAGE_FAMILY = {STAGE_ONE_ROW: "one_row", STAGE_TILES: "tiles", STAGE_ROWS_IN_REGISTERS: "rows_in_registers",
                STAGE_GROUPS_OF_8: "groups_of_8", STAGE_REFUSED: "refused"}
STAGE_LAUNCHER = {STAGE_ONE_ROW: "row_gemv1", STAGE_TILES: "row_mfma", STAGE_ROWS_IN_REGISTERS: "row_gemvm",
                  STAGE_GROUPS_OF_8: "row_linear_8"}
F_LN, F_RES, F_RES_LN, F_RELU = 1, 2, 4, 8                    # DecodeStageCase.flags
KV_NONE, KV_F32, KV_BF16 = 0, 1, 2                            # .kv: no out2 (split == N) | fp32 out2 | bf16 out2
AT_VALUE, AT_COUNTER, AT_ROWS, AT_ROWS_COUNTER = 0, 1, 2, 3   # .addr: by value | device counter | row_pos direct | beside the counter
WS_NONE, WS_GIVEN, WS_SHORT = 0, 1, 2                         # .ws: the tile workspace: none | given | one float short
H_NONE, H_STAT_OUT, H_RES_STAT = 0, 1, 2                      # .handoff bits
# part = (heads, head_dim, splits, kind): kind 0 plain | 1 split 1 of every head is neutral | 2 split 0 lies 60 below the others
DecodeStageCase = collections.namedtuple("DecodeStageCase", "M N K split flags kv addr ws mfma_rows stats_global part handoff kernel")


def _dsc(kernel, M, N, K, split=None, flags=F_LN, kv=KV_NONE, addr=AT_VALUE, ws=WS_NONE, mfma_rows=16, stats_global=0, part=None,
         handoff=H_NONE):
    split = N if kv == KV_NONE else split
    return DecodeStageCase(M, N, K, split, flags, kv, addr, ws, mfma_rows, stats_global, part, handoff, kernel)


def decode_stage_case_id(c):
    h, hd, ns, kind = c.part or (0, 0, 0, 0)
    return (f"stagex/m{c.M}/n{c.N}/k{c.K}/s{c.split}/f{c.flags}/v{c.kv}/a{c.addr}/w{c.ws}/q{c.mfma_rows}.{c.stats_global}/"
            f"g{h}.{hd}.{ns}.{kind}/h{c.handoff}")


def _decode_stage_table():
    t = []
    ALL = F_LN | F_RES | F_RES_LN | F_RELU
    flag_cycle = (ALL, F_LN, F_LN | F_RES | F_RES_LN, F_LN | F_RES | F_RELU, 0, F_RES)
    # ---- the one-row kernel: the four KQ on both sides of each threshold; k|v with an odd split, fp32 and bf16; N around the
    # 8 (KQ <= 2) / 4 (KQ >= 4) features of a workgroup; position by value and by the counter; the hand-off both ways
    for i, K in enumerate((64, 256, 260, 512, 516, 1024, 1028, 2048)):
        for kv in (KV_F32, KV_BF16):
            t.append(_dsc(STAGE_ONE_ROW, 1, 40, K, 7, flag_cycle[i % 6] | F_LN, kv, AT_COUNTER if (i + kv) & 1 else AT_VALUE))
    for K in (64, 1028):
        for N in (1, 7, 8, 9):
            t.append(_dsc(STAGE_ONE_ROW, 1, N, K, flags=ALL if N != 8 else F_RES, addr=AT_COUNTER if N == 9 else AT_VALUE))
            if N > 1:
                t.append(_dsc(STAGE_ONE_ROW, 1, N, K, 3, F_LN, KV_BF16 if N == 8 else KV_F32))
    for K in (256, 1024):
        t.append(_dsc(STAGE_ONE_ROW, 1, 40, K, flags=F_LN | F_RELU, handoff=H_STAT_OUT))
        t.append(_dsc(STAGE_ONE_ROW, 1, 40, K, flags=F_RES | F_RES_LN, handoff=H_RES_STAT, addr=AT_COUNTER))
    # merged input: the out-projection of a batch-1 step (normalised residual, on and off the hand-off)
    for j, part in enumerate(((4, 16, 1, 0), (2, 32, 3, 0), (8, 32, 2, 1), (4, 64, 8, 2), (8, 64, 3, 1), (16, 32, 8, 0), (8, 64, 2, 2))):
        t.append(_dsc(STAGE_ONE_ROW, 1, 40, part[0] * part[1], flags=F_RES | F_RES_LN, part=part, addr=AT_COUNTER if j & 1 else AT_VALUE,
                      handoff=H_RES_STAT if j % 3 == 2 else H_NONE))
    # ---- rows in registers: the nine (KQ, MR), a ragged last group, row_pos on and off, fp32 and bf16 k|v
    for i, (K, M) in enumerate(((256, 2), (256, 3), (256, 8), (256, 9), (260, 4), (260, 5), (260, 17), (512, 2), (512, 5), (516, 2),
                                (516, 3), (516, 9), (1024, 4), (1028, 2), (1028, 3), (2048, 5))):
        for addr in (AT_COUNTER if i & 1 else AT_VALUE, AT_ROWS_COUNTER if i & 1 else AT_ROWS):
            for kv in (KV_F32, KV_BF16):
                t.append(_dsc(STAGE_ROWS_IN_REGISTERS, M, 24, K, 7, flag_cycle[i % 6] | F_LN, kv, addr))
    for M, addr in ((3, AT_VALUE), (9, AT_ROWS)):
        t.append(_dsc(STAGE_ROWS_IN_REGISTERS, M, 24, 512, flags=F_LN, handoff=H_STAT_OUT, addr=addr))
        t.append(_dsc(STAGE_ROWS_IN_REGISTERS, M, 24, 512, flags=ALL & ~F_LN, handoff=H_RES_STAT, addr=addr))
    # ---- 32-row tiles: M around a tile, N around a tile with the k|v boundary inside it, K in one chunk / a short last chunk /
    # four chunks; the chunks side by side (workspace), one after the other (none), a workspace one float short
    for M in (2, 31, 32, 33, 40):
        t.append(_dsc(STAGE_TILES, M, 33, 512, 16, ALL, KV_F32, mfma_rows=1 if M == 2 else 16, ws=WS_GIVEN))
    for N in (31, 32, 48):
        t.append(_dsc(STAGE_TILES, 33, N, 512, 16, F_LN | F_RES, KV_BF16, ws=WS_GIVEN))
    for K in (8, 520, 2048):
        for ws in (WS_GIVEN, WS_NONE, WS_SHORT):
            t.append(_dsc(STAGE_TILES, 33, 48, K, 16, ALL, KV_BF16 if ws == WS_GIVEN else KV_F32, ws=ws,
                          addr=AT_COUNTER if ws == WS_GIVEN else AT_VALUE))
    for K in (8, 512):                                   # the statistics from memory where the staged tile would give them
        t.append(_dsc(STAGE_TILES, 33, 48, K, 16, ALL, KV_F32, stats_global=1))
    for K, ws in ((512, WS_NONE), (2048, WS_GIVEN), (2048, WS_NONE)):
        for kv in (KV_F32, KV_BF16):
            t.append(_dsc(STAGE_TILES, 33, 48, K, 16, ALL, kv, AT_ROWS if kv == KV_F32 else AT_ROWS_COUNTER, ws))
    for K, ws, sg in ((512, WS_NONE, 0), (512, WS_NONE, 1), (2048, WS_GIVEN, 0), (2048, WS_NONE, 0)):
        t.append(_dsc(STAGE_TILES, 33, 48, K, flags=F_LN, handoff=H_STAT_OUT, ws=ws, stats_global=sg))
        t.append(_dsc(STAGE_TILES, 33, 48, K, flags=F_RES | F_RES_LN, handoff=H_RES_STAT, ws=ws, addr=AT_ROWS if sg else AT_VALUE))
    # a normalised residual of 516 features: on the tiles with its statistics handed (8 residual floats per lane and row are what
    # the tile kernel reduces itself); without them the plan leaves the tiles -- five groups of 8, or refused with row_pos
    for K, ws in ((512, WS_NONE), (2048, WS_GIVEN)):
        t.append(_dsc(STAGE_TILES, 33, 516, K, flags=F_RES | F_RES_LN, ws=ws, handoff=H_RES_STAT))
        t.append(_dsc(STAGE_GROUPS_OF_8, 33, 516, K, flags=F_RES | F_RES_LN, ws=ws))
    t.append(_dsc(STAGE_TILES, 33, 516, 512, flags=F_RES | F_RES_LN, addr=AT_ROWS, handoff=H_RES_STAT))
    t.append(_dsc(STAGE_REFUSED, 33, 516, 512, flags=F_RES | F_RES_LN, addr=AT_ROWS))
    # ---- groups of 8 rows in LDS: the four row capacities, two launches at 9 rows, the K tail beyond 8 float4 per lane
    for i, M in enumerate((1, 2, 3, 4, 5, 8, 9)):
        for K in (2052, 2560):
            t.append(_dsc(STAGE_GROUPS_OF_8, M, 24, K, 7, flag_cycle[i % 6] | F_LN, KV_BF16 if (i + K // 4) & 1 else KV_F32,
                          AT_COUNTER if i % 3 == 0 else AT_VALUE))
    for N, M in ((516, 1), (516, 3), (1024, 1), (1024, 9)):
        t.append(_dsc(STAGE_GROUPS_OF_8, M, N, 512, flags=ALL, addr=AT_COUNTER if M == 3 else AT_VALUE))
    # 17 rows of K = 2056: on the tiles (a short fifth chunk) without a LayerNorm; with one, whose statistics the tiles form for
    # K <= 2048 only, in three groups of 8
    t.append(_dsc(STAGE_TILES, 17, 24, 2056, flags=F_RES | F_RELU))
    t.append(_dsc(STAGE_GROUPS_OF_8, 17, 24, 2056, flags=F_LN | F_RES))
    t.append(_dsc(STAGE_GROUPS_OF_8, 8, 24, 5116, flags=F_LN))        # 8 rows of 5116 floats: the last that fit in 160 KiB with
    t.append(_dsc(STAGE_REFUSED, 8, 24, 5120, flags=F_LN))            # ... their statistics; beyond the LDS bound: refused
    t.append(_dsc(STAGE_REFUSED, 3, 24, 2052, 7, F_LN, KV_F32, AT_ROWS))   # per-row positions where no batched kernel takes K
    return t


DECODE_STAGE_CASES = _decode_stage_table()


def decode_stage_instance(c):
    """The template instantiation(s) the launchers of csrc/prior_decode.hip pick for a case, from its shape alone."""
    kq = 1 if c.K <= 256 else 2 if c.K <= 512 else 4 if c.K <= 1024 else 8
    kv16, rag = c.kv == KV_BF16, c.addr in (AT_ROWS, AT_ROWS_COUNTER)
    if c.kernel == STAGE_ONE_ROW:
        return ("row_gemv1", kq, kv16, c.part is not None)
    if c.kernel == STAGE_ROWS_IN_REGISTERS:
        mr = 2 if c.M <= 2 else 4 if c.M <= 4 else 8
        while kq * mr > 16:
            mr //= 2
        return ("row_gemvm", kq, mr, rag, kv16)
    if c.kernel == STAGE_TILES:
        nz, tiles = -(-c.K // 512), -(-c.N // 32) * -(-c.M // 32)
        side_by_side = nz > 1 and tiles < 128 and c.ws == WS_GIVEN
        stats = "none" if not c.flags & F_LN else "staged" if c.K <= 512 and not c.stats_global else "memory"
        return ("row_mfma32", rag, kv16, side_by_side, stats)
    if c.kernel == STAGE_GROUPS_OF_8:
        groups = [min(8, c.M - m0) for m0 in range(0, c.M, 8)]
        return ("row_linear_ln", tuple(1 if g <= 1 else 2 if g <= 2 else 4 if g <= 4 else 8 for g in groups), kv16)
    return ("refused",)


def decode_stage_coverage_gaps(cases):
    """What `cases` leave out of the template instantiations the launchers of csrc/prior_decode.hip can pick: [] when every
    KQ x KV16 of the one-row kernel (and the merged input at both KQ it exists for), every (KQ, MR) x RAG x KV16 of the
    rows-in-registers kernel, RAG x KV16 x (chunks side by side with the finishing launch | not) and the three forms of the
    input statistics of the tiles, and every MR x KV16 of the LDS kernel (two launches at 9 rows) occur."""
    inst = collections.Counter(decode_stage_instance(c) for c in cases)
    want = [("row_gemv1", kq, kv16, False) for kq in (1, 2, 4, 8) for kv16 in (False, True)]
    want += [("row_gemv1", 1, False, True), ("row_gemv1", 2, False, True)]
    want += [("row_gemvm", kq, mr, rag, kv16) for kq, mr in ((1, 2), (1, 4), (1, 8), (2, 2), (2, 4), (2, 8), (4, 2), (4, 4), (8, 2))
             for rag in (False, True) for kv16 in (False, True)]
    gaps = [w for w in want if not inst[w]]
    gaps += [("row_mfma32", rag, kv16, side) for rag in (False, True) for kv16 in (False, True) for side in (False, True)
             if not any(k[:4] == ("row_mfma32", rag, kv16, side) for k in inst)]
    gaps += [("row_mfma32 statistics", f) for f in ("none", "staged", "memory") if not any(k[0] == "row_mfma32" and k[4] == f for k in inst)]
    gaps += [("row_linear_ln", mr, kv16) for mr in (1, 2, 4, 8) for kv16 in (False, True)
             if not any(k[0] == "row_linear_ln" and k[2] == kv16 and mr in k[1] for k in inst)]
    gaps += [("row_linear_ln", "two launches")] if not any(k[0] == "row_linear_ln" and len(k[1]) == 2 for k in inst) else []
    return gaps


def decode_stage_row_positions(M, own=True):
    """row_pos [2 steps][M]: at step DECODE_STAGE_P row m stands at its own position (own) or every row at DECODE_STAGE_P; the
    other step holds other valid positions, so a kernel reading the wrong step reads rows that hold NaN."""
    P = DECODE_STAGE_POSITIONS
    at = [(2 * m + 1) % P if own else DECODE_STAGE_P for m in range(M)]
    other = [(a + 1) % P for a in at]
    rows = [other, at] if DECODE_STAGE_P == 1 else [at, other]
    return torch.tensor(rows, dtype=torch.int32)


def decode_stage_data(c, seed=None):
    """The tensors of a case on the CPU, float32: x [P][M][K] and res [P][M][N] at every position (rows differ in scale and
    offset, so a neighbour's statistics do not fit), W [N][K], bias, the LayerNorm parameters, the attention partials."""
    g = torch.Generator().manual_seed(seed if seed is not None else 1000003 * c.M + 1009 * c.N + c.K + 17 * c.flags + c.addr)
    P, M, N, K = DECODE_STAGE_POSITIONS, c.M, c.N, c.K
    rnd = lambda *s: torch.randn(*s, generator=g)
    d = {}
    scale = 0.5 + 1.5 * torch.rand(P, M, 1, generator=g)
    d["x"] = rnd(P, M, K) * scale + (2.0 * torch.rand(P, M, 1, generator=g) - 1.0)
    d["W"] = rnd(N, K) / math.sqrt(K)
    d["bias"] = rnd(N)
    d["ln_g"], d["ln_b"] = 1 + 0.1 * rnd(K), 0.1 * rnd(K)
    d["res"] = rnd(P, M, N) * (0.5 + 1.5 * torch.rand(P, M, 1, generator=g)) + (2.0 * torch.rand(P, M, 1, generator=g) - 1.0)
    d["res_g"], d["res_b"] = 1 + 0.1 * rnd(N), 0.1 * rnd(N)
    if c.part:
        H, HD, NS, kind = c.part
        part = torch.zeros(H, NS, HD + 4)
        part[:, :, :HD] = rnd(H, NS, HD)
        part[:, :, HD] = 3.0 * rnd(H, NS)                                   # the split's maximum logit
        part[:, :, HD + 1] = 0.5 + 1.5 * torch.rand(H, NS, generator=g)     # its sum of exp(logit - maximum)
        if kind == 1:                        # what the attention kernel writes for a split without keys
            part[:, 1, :HD], part[:, 1, HD], part[:, 1, HD + 1] = 0.0, -1e30, 0.0
        if kind == 2:
            part[:, 0, HD] = part[:, 1:, HD].amax(dim=1) - 60.0
        d["part"] = part
    return d


def decode_stage_rows(c, d, row_pos=None):
    """(x rows [M][K], residual rows [M][N]) the case addresses: position DECODE_STAGE_P, or row m at row_pos[DECODE_STAGE_P][m]."""
    at = [DECODE_STAGE_P] * c.M if row_pos is None else [int(v) for v in row_pos[DECODE_STAGE_P]]
    m = torch.arange(c.M)
    return d["x"][at, m], d["res"][at, m]


def row_stats(rows, eps, dtype=torch.float64, pad_to=None):
    """[M][2]: (mean, 1 / sqrt(biased variance + eps)) per row.  Mutants: `pad_to`, the variance also sums (0 - mean)^2 over the
    lanes between the width and its next multiple of pad_to (a missing bounds check in the second pass)."""
    z = rows.to(dtype)
    D = z.shape[-1]
    mean = z.sum(dim=-1, keepdim=True) / D
    sq = (z - mean).pow(2).sum(dim=-1, keepdim=True)
    if pad_to:
        sq = sq + (-(-D // pad_to) * pad_to - D) * mean * mean
    return torch.cat([mean, 1.0 / torch.sqrt(sq / D + eps)], dim=-1)


def _normalise(rows, stats, gamma, beta):
    return (rows - stats[:, :1]) * stats[:, 1:] * gamma + beta


def decode_stage_eval(dtype, x, W, bias=None, ln=None, res=None, res_ln=None, relu=False, eps=1e-5, split=None, res_stats=None,
                      stat_perm=None, res_stat_perm=None, pad_to=None, k_keep=None, out2_shift=0):
    """(out [M][split], out2 [M][N - split] or None, the input rows' statistics [M][2] or None) of a stage in `dtype`:
    act(LN(x) W^T + bias + LN_res(res)), LayerNorm statistics (mean, 1 / sqrt(var + eps)) per row; `res_stats` [M][2]: the
    residual's statistics as given.  The mutants of the host tests: stat_perm / res_stat_perm, row m is normalised with the
    statistics of row perm[m]; pad_to (row_stats); k_keep, the products beyond k_keep are dropped; out2_shift, out2's columns
    rolled by that many."""
    t = lambda v: None if v is None else torch.as_tensor(v).detach().cpu().to(dtype)
    x, W, bias, res = t(x), t(W), t(bias), t(res)
    stats = None
    if ln is not None:
        stats = row_stats(x, eps, dtype, pad_to=pad_to)
        x = _normalise(x, stats if stat_perm is None else stats[stat_perm], t(ln[0]), t(ln[1]))
    y = x @ W.t() if k_keep is None else x[:, :k_keep] @ W[:, :k_keep].t()
    if bias is not None:
        y = y + bias
    if res is not None:
        if res_ln is not None:
            rs = row_stats(res, eps, dtype, pad_to=pad_to) if res_stats is None else t(res_stats)
            res = _normalise(res, rs if res_stat_perm is None else rs[res_stat_perm], t(res_ln[0]), t(res_ln[1]))
        y = y + res
    if relu:
        y = y.clamp(min=0.0)
    split = y.shape[1] if split is None else split
    out2 = y[:, split:] if split < y.shape[1] else None
    if out2 is not None and out2_shift:
        out2 = out2.roll(out2_shift, dims=1)
    return y[:, :split], out2, stats


def decode_stage_spec(*a, **kw):
    return decode_stage_eval(torch.float64, *a, **kw)


def decode_stage_f32(*a, **kw):
    return decode_stage_eval(torch.float32, *a, **kw)


def merge_partials_eval(dtype, part, splits=None, subtract_max=True):
    """The input row [H * HD] from an attention's key-split partials [H][NS][HD + 4] = (o[HD], max, sum, -, -):
    M = max_s max_s, w_s = exp(max_s - M), x = sum_s w_s o_s / sum_s w_s sum_s.  Mutants: `splits`, only the first that many
    are merged; subtract_max=False, w_s = exp(max_s)."""
    p = torch.as_tensor(part).detach().cpu().to(dtype)
    HD = p.shape[2] - 4
    p = p[:, :splits] if splits else p
    mx = p[:, :, HD]
    w = torch.exp(mx - mx.amax(dim=1, keepdim=True)) if subtract_max else torch.exp(mx)
    num = (w.unsqueeze(-1) * p[:, :, :HD]).sum(dim=1)
    den = (w * p[:, :, HD + 1]).sum(dim=1, keepdim=True)
    return (num / den).reshape(1, -1)


def merge_partials_spec(part):
    return merge_partials_eval(torch.float64, part)


def merge_partials_f32(part, **kw):
    return merge_partials_eval(torch.float32, part, **kw)


def single_source_eval(dtype, y1, gamma, beta, table, pos, Cd, eps=1e-5, with_stats=True):
    """(y2 [B][d], its statistics [B][2]) of the single-source cross-attention block: y2[m] = LN1(y1[m]) + table[pos[m] // Cd][m]
    for a table [S_src][B or 1][d] (one row per source position: shared by all rows)."""
    t = lambda v: torch.as_tensor(v).detach().cpu().to(dtype)
    y1, table = t(y1), t(table)
    B = y1.shape[0]
    src = torch.stack([table[int(pos[m]) // Cd, m if table.shape[1] > 1 else 0] for m in range(B)])
    y2 = _normalise(y1, row_stats(y1, eps, dtype), t(gamma), t(beta)) + src
    return y2, (row_stats(y2, eps, dtype) if with_stats else None)


def single_source_spec(*a, **kw):
    return single_source_eval(torch.float64, *a, **kw)


def single_source_f32(*a, **kw):
    return single_source_eval(torch.float32, *a, **kw)


def bf16_widen(bits):
    """int16 bf16 patterns -> float32."""
    return (torch.as_tensor(bits).cpu().to(torch.int32) << 16).view(torch.float32)


def bf16_bits(v, truncate=False):
    """float32 -> int16 bf16 patterns, rounded to nearest-even (the mutant: truncated)."""
    v = torch.as_tensor(v).detach().cpu().float().contiguous()
    if truncate:
        return (v.view(torch.int32) >> 16).to(torch.int16)
    return v.to(torch.bfloat16).view(torch.int16)


def compare_rows_bf16(got, ref, yardstick, what, margin=ROW_OPS_MARGIN):
    """compare_rows for values stored as bf16 (`got`: widened): every element within the fp32 bound of its row --
    margin * max(row_error(yardstick, ref), 2^-23) * max|ref_row| -- plus half a bf16 ulp of the spec value (8 bits of
    significand: 2^(exponent - 8)).  ratio: the part of the error beyond the half ulp against the yardstick."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{what}: shape or a non-finite value"
    yard = max(row_error(yardstick, ref), ROW_OPS_FLOOR)
    assert math.isfinite(yard), f"{what}: the float32 yardstick itself is not finite"
    half_ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -126))) - 8.0)
    scale = ref.abs().amax(dim=-1, keepdim=True).clamp(min=2.0 ** -100)
    beyond = (((got - ref).abs() - half_ulp).clamp(min=0.0) / scale).max()
    err, ratio = float(((got - ref).abs() / scale).max()), float(beyond) / yard
    assert ratio <= margin, (f"{what}: {float(beyond):.3e} beyond half a bf16 ulp is {ratio:.1f} times the float32 yardstick "
                             f"{yard:.3e} (margin {margin:g})")
    return RowCheck(what, err, yard, ratio)


# isi_decode_single_source_f32: (d, B, Cd, shared table, addressing, stat_out)
SingleSourceCase = collections.namedtuple("SingleSourceCase", "d B Cd shared addr stats")
SINGLE_SOURCE_CASES = [SingleSourceCase(*v) for v in (
    (64, 1, 1, False, AT_VALUE, True), (64, 3, 4, True, AT_COUNTER, True), (64, 4, 4, False, AT_ROWS, True),
    (64, 5, 1, False, AT_ROWS_COUNTER, False), (100, 1, 4, True, AT_COUNTER, False), (100, 3, 1, False, AT_ROWS, False),
    (100, 4, 4, True, AT_VALUE, True), (100, 5, 4, False, AT_ROWS_COUNTER, True), (1024, 1, 4, False, AT_COUNTER, True),
    (1024, 3, 4, False, AT_VALUE, False), (1024, 4, 1, True, AT_ROWS_COUNTER, True), (1024, 5, 4, True, AT_ROWS, True))]
SINGLE_SOURCE_P = 5              # the position / step addressed; rows of a ragged launch stand at SINGLE_SOURCE_P - (m % 3) * 2
SINGLE_SOURCE_S_SRC = 6


def single_source_positions(c, own=True):
    """[steps = SINGLE_SOURCE_P + 1][B] positions; the step addressed is the last."""
    at = [SINGLE_SOURCE_P - ((m % 3) * 2 if own else 0) for m in range(c.B)]
    return torch.tensor([[(a + 1 + t) % (SINGLE_SOURCE_P + 1) for a in at] for t in range(SINGLE_SOURCE_P)] + [at], dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# Float64 specification, float32 yardstick and 16-bit operand models of the training-side relative attention FORWARD
# (isi_rel_attention_f32: csrc/rel_attention_f32.hip, rel_attention_fwd2.hip, rel_attention_fwd3.hip, routed by
# attn_fwd_route in csrc/rel_attention_run.cpp), in the style of the blocks above: plain torch on the CPU, no autograd
# and none of the project's kernels.  include/isi_hip.h (isi_attn_args) states the operation:
#     logit[i,j] = (q_i.k_j + q_i.e[h, r(i,j)]) * scale + mask(i,j),   r(i,j) = floor(i/Cq) - floor(j/Ck) + Ek - 1
#     out_i = softmax_j(logit) v_j over the pairs mask_mode allows;  lse_i = log sum_j exp(logit)   (natural log)
#     kept logits (16-bit modes): logit * log2(e) of every allowed pair
#     a row with no allowed pair, or with only -inf logits (an EMPTY row): out = 0, lse = 1e30f
# Tensors here: q [Sq,B,H,hd] (or [Sq,B,H*hd]), k / v [Sk,B,H,hd], the table [H,rel_rows,hd] or None, the dense additive
# mask [Sq,Sk] or None; results out [B,H,Sq,hd], lse [B,H,Sq], logits2 [B,H,Sq,Sk], allowed [Sq,Sk].
# tests/test_attention_fwd_host.py holds the spec to oracle/prior_oracle.py and shows what the hold rejects;
# tests/test_attention_fwd_gpu.py holds every kernel route to it.
ATTN_QB = 128                                  # QB of csrc/rel_attention.h: query rows per block
ATTN_LOG2E = 1.4426950408889634
ATTN_EMPTY_LSE = float(np.float32(1e30))       # what the kernels store as the log-sum-exp of an empty row
ATTN_FAMILIES = ("exact", "tiles64", "planes")
ATTN_KNOB_NO_FWD3, ATTN_KNOB_FWD3_ALL = 1, 2   # bits of `knobs`, as in tests/attention_plan_tracer.cpp
ATTN_KNOB_NAMES = {ATTN_KNOB_NO_FWD3: "ISI_ATTN_NO_FWD3", ATTN_KNOB_FWD3_ALL: "ISI_ATTN_FWD3_ALL"}
AttnFwd = collections.namedtuple("AttnFwd", "out lse logits2 allowed")


def attention_allowed(Sq, Sk, mask_mode, strict=False):
    """The [Sq,Sk] predicate of mask_mode: 0 every pair, 1 causal (j <= i), 2 anti-causal (j >= i).  `strict` is a host-test
    mutant (j < i, j > i)."""
    i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    if mask_mode == 1:
        return (j < i) if strict else (j <= i)
    if mask_mode == 2:
        return (j > i) if strict else (j >= i)
    assert mask_mode == 0, mask_mode
    return torch.ones(Sq, Sk, dtype=torch.bool)


def attention_rel_index(Sq, Sk, Cq, Ck, Ek):
    """r(i,j) = floor(i/Cq) - floor(j/Ck) + Ek - 1, [Sq,Sk]."""
    return torch.arange(Sq)[:, None] // Cq - torch.arange(Sk)[None, :] // Ck + (Ek - 1)


def _attn_heads(t, H):
    """[S,B,H,hd] or [S,B,H*hd] -> [B,H,S,hd]"""
    t = torch.as_tensor(t).detach().cpu()
    if t.dim() == 3:
        t = t.reshape(t.shape[0], t.shape[1], H, t.shape[2] // H)
    return t.permute(1, 2, 0, 3)


def _attn_softmax(l2, allowed, pv, dtype, lse_base2=False, drop_last_key=False, stale_max=False):
    """Softmax over the allowed, finite base-2 logits of every row, the product with V through `pv(p)`, the log-sum-exp
    and the empty-row convention.  The switches are the host tests' mutants: `drop_last_key` leaves the last key of a
    ragged 32-key tile (Sk % 32 != 0) out of the softmax; `stale_max` is an online softmax over [the keys before the last
    32-key tile | that tile] that forgets to rescale the first part's numerator when the last tile raises the maximum."""
    Sk = l2.shape[-1]
    ninf = torch.tensor(float("-inf"), dtype=dtype)
    if drop_last_key and Sk % 32:
        allowed = allowed.clone()
        allowed[:, Sk - 1] = False
    masked = torch.where(allowed, l2, ninf)
    m = masked.amax(dim=-1, keepdim=True)
    empty = m == float("-inf")
    msafe = torch.where(empty, torch.zeros_like(m), m)
    p = torch.exp2(masked - msafe)
    l = p.sum(dim=-1, keepdim=True)
    num = pv(p)
    if stale_max and Sk > 32:
        cut = (Sk - 1) // 32 * 32
        m0 = masked[..., :cut].amax(dim=-1, keepdim=True)
        has0 = m0 > float("-inf")
        # the first part's numerator relative to ITS maximum, never rescaled by alpha = exp2(m0 - m)
        first = torch.where(has0, torch.exp2(masked[..., :cut] - torch.where(has0, m0, torch.zeros_like(m0))), torch.zeros_like(p[..., :cut]))
        num = pv(torch.cat([first, p[..., cut:]], dim=-1))
    one = torch.ones_like(l)
    out = torch.where(empty, torch.zeros_like(num), num / torch.where(empty, one, l))
    lse = msafe + torch.log2(torch.where(empty, one, l))
    if not lse_base2:
        lse = lse * math.log(2.0)
    lse = torch.where(empty, torch.full_like(lse, ATTN_EMPTY_LSE), lse)
    return out, lse.squeeze(-1)


def _attention_eval(dtype, q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, rel_shift=0, swap_c=False, strict_causal=False,
                    rel_unscaled=False, dense_on_disallowed=False, lse_base2=False, logits_no_mask=False, drop_last_key=False,
                    stale_max=False):
    """The operation in `dtype`; every keyword is a mutant of the host tests (off: the operation as specified)."""
    hq, hk, hv = (_attn_heads(t, H).to(dtype) for t in (q, k, v))
    Sq, Sk = hq.shape[2], hk.shape[2]
    s = hq @ hk.transpose(-1, -2)
    if rel is not None:
        e = torch.as_tensor(rel).detach().cpu().to(dtype)
        idx = attention_rel_index(Sq, Sk, *((Ck, Cq) if swap_c else (Cq, Ck)), Ek) + rel_shift
        if rel_shift or swap_c:
            idx = idx.clamp(0, e.shape[1] - 1)
        assert int(idx.min()) >= 0 and int(idx.max()) < e.shape[1], "the table must cover every (query, key) pair"
        srel = torch.einsum("bhid,hrd->bhir", hq, e).gather(3, idx.expand(hq.shape[0], H, Sq, Sk))
        s = (s * scale + srel) if rel_unscaled else (s + srel) * scale
    else:
        s = s * scale
    l2 = s * ATTN_LOG2E
    allowed = attention_allowed(Sq, Sk, mask_mode)
    used = attention_allowed(Sq, Sk, mask_mode, strict=True) if strict_causal else allowed
    kept = l2
    if dense_mask is not None:
        dm = torch.as_tensor(dense_mask).detach().cpu().to(dtype) * ATTN_LOG2E
        with_mask = l2 + (torch.where(used, torch.zeros_like(dm), dm) if dense_on_disallowed else dm)
        kept = l2 if logits_no_mask else with_mask
        l2 = with_mask
    out, lse = _attn_softmax(l2, used, lambda p: p @ hv, dtype, lse_base2, drop_last_key, stale_max)
    return AttnFwd(out, lse, kept, allowed)


def attention_fwd_spec(q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale):
    """The float64 specification: (out, lse, logits2, allowed).  logits2 = (q.k + q.e[r]) * scale * log2(e) + mask * log2(e)
    for every pair (the entries `allowed` leaves out are unspecified in a kernel's buffer); a pair whose dense-mask entry is
    -inf is allowed, has weight 0 and logit -inf; an empty row has out = 0 and lse = ATTN_EMPTY_LSE."""
    return _attention_eval(torch.float64, q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale)


def attention_fwd_f32(q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, **mutant):
    """The same evaluation in float32 torch on the CPU: the yardstick (and what the host tests mutate)."""
    return _attention_eval(torch.float32, q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, **mutant)


def _attn_pieces(t, precision):
    """The float64 values of the 16-bit pieces a kernel makes of the float32 tensor t: precision 1 (hi, lo) =
    bf16_pieces(t, 2); 2 (rne_bf16(t),); 3 (rne_f16(t),)."""
    t = t.float()
    if precision == 1:
        return bf16_pieces(t, 2)
    if precision == 2:
        return (t.bfloat16().double(),)
    assert precision == 3, precision
    assert float(t.abs().max()) < 65504.0, "outside f16's range (include/isi_hip.h: |q k v e| < 65504)"
    return (t.half().double(),)


def _attn_terms(A, Bp, contract, drop=None):
    """The products a mode keeps of (pieces A of K / e / V) x (pieces Bp of Q / P): one term for the single-term modes,
    A.lo B.hi + A.hi B.lo + A.hi B.hi for precision 1.  `drop` = "lo_hi" (the A.lo B.hi term) is a host-test mutant."""
    if len(A) == 1:
        return contract(A[0], Bp[0])
    s = contract(A[0], Bp[0]) + contract(A[0], Bp[1])
    return s if drop == "lo_hi" else s + contract(A[1], Bp[0])


def attention_fwd_model(q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, precision, drop=None):
    """Float64 evaluation on the operands the 16-bit kernels multiply; its distance from the spec is the truncation the mode
    accepts by design.  Read from csrc/rel_attention_fwd2.hip (rel_attention_fwd3.hip computes the same products from planes
    attn_pack_kernel makes with the same conversions, lines 128-138):
      * q is multiplied by qscale = scale * log2(e) in float32 and THEN converted (fwd2 lines 112, 263-276; fwd3 lines 210,
        375-390): `PR::split2(a.x * qscale, ...)` for precision 1, `PR::pack2(a.x * qscale, ...)` for 2 and 3;
      * K and the table rows are converted as they are (fwd2 `put_row`, lines 174-185; fwd3's pack kernel);
      * S^T = K Q^T and the band product E Q^T keep `mfma(k_lo, q_hi); mfma(k_hi, q_lo); mfma(k_hi, q_hi)` (fwd2 lines
        341-356, fwd3 lines 500-503 and 527-531), one product for the single-term modes; float32 accumulation;
      * the dense mask is added in float32 as mask * log2(e) (fwd2 line 434), the softmax runs in float32 on base-2 logits;
      * the row sum l adds the float32 probabilities BEFORE their conversion (fwd2 lines 419-420, 457-459), the numerator
        multiplies converted probabilities with converted V (fwd2 lines 468-483: `PR::split2(sv[...])` / `PR::pack2`; V in
        `commit`, lines 194-212) and keeps `mfma(v_lo, p_hi); mfma(v_hi, p_lo); mfma(v_hi, p_hi)` (lines 500-505).
    Conversions round to nearest even (`__builtin_convertvector`); hi = rne(x), lo = rne(x - hi) (csrc/split_bf16.h).  The
    model converts the probabilities relative to the row's FINAL maximum where the kernels convert them relative to the
    running one and rescale afterwards: the same relative rounding, at another power of two.  `drop`: a host-test mutant."""
    assert precision in (1, 2, 3), precision
    hq, hk, hv = (_attn_heads(t, H).float() for t in (q, k, v))
    Sq, Sk = hq.shape[2], hk.shape[2]
    qscale = np.float32(scale) * np.float32(ATTN_LOG2E)
    Q = _attn_pieces(hq * float(qscale), precision)
    l2 = _attn_terms(_attn_pieces(hk, precision), Q, lambda a, b: b @ a.transpose(-1, -2), drop)
    if rel is not None:
        e = torch.as_tensor(rel).detach().cpu().float()
        idx = attention_rel_index(Sq, Sk, Cq, Ck, Ek)
        assert int(idx.min()) >= 0 and int(idx.max()) < e.shape[1]
        band = _attn_terms(_attn_pieces(e, precision), Q, lambda a, b: torch.einsum("bhid,hrd->bhir", b, a), drop)
        l2 = l2 + band.gather(3, idx.expand(hq.shape[0], H, Sq, Sk))
    if dense_mask is not None:
        l2 = l2 + torch.as_tensor(dense_mask).detach().cpu().double() * ATTN_LOG2E
    allowed = attention_allowed(Sq, Sk, mask_mode)
    V = _attn_pieces(hv, precision)
    out, lse = _attn_softmax(l2, allowed, lambda p: _attn_terms(V, _attn_pieces(p, precision), lambda a, b: b @ a, drop), torch.float64)
    return AttnFwd(out, lse, l2, allowed)


def attention_tail_rows(S, mask_mode, dense):
    """attention_tail_rows of csrc/rel_attention_run.cpp"""
    tail = S % ATTN_QB
    return tail if (1 <= tail <= 2 and S >= 2 * ATTN_QB and not dense and mask_mode == 0) else 0


def attention_fwd_route(hd, precision, Cq, Ck, table, Sq, mask_mode, dense, workspace, knobs, cus, B, H, Sk=None, rel_rows=None):
    """Restatement of attn_fwd_route, attention_tail_rows, blocks and persistent_workgroups (csrc/rel_attention_run.cpp):
    (family, tail_rows, nW) of an accepted forward call.  workspace: "none" | "given" | "query" (the caller brings one iff
    isi_rel_attention_workspace_bytes answers > 0); knobs: bits ATTN_KNOB_*; cus: the device's CU count.  family "exact"
    (precision 0; nW = its grid's query blocks), "tiles64" (rel_attention_fwd2.hip) or "planes" (rel_attention_fwd3.hip);
    tail_rows: rows the one-row kernel takes behind a 16-bit kernel; nW: persistent workgroups per (batch, head) pair.  With
    Sk and rel_rows the planes' 2 GiB limit (planes_ok) is applied too."""
    assert workspace in ("none", "given", "query"), workspace
    cdiv = lambda a, b: (a + b - 1) // b
    if precision == 0:
        return "exact", 0, cdiv(Sq, ATTN_QB)
    planes_ok = Cq == 1 and Ck == 1 and hd in (32, 64) and 1 <= precision <= 3 and bool(table)
    if planes_ok and Sk is not None:
        npl = 2 if precision == 1 else 1
        planes_ok = (npl * H * B * cdiv(Sk, 32) * 32 * hd * 2 < 2 ** 31 and npl * H * (rel_rows or 0) * hd * 2 < 2 ** 31)
    if workspace == "query" and precision != 1 and not knobs & ATTN_KNOB_FWD3_ALL:
        family = "tiles64"
    elif workspace == "none" or knobs & ATTN_KNOB_NO_FWD3 or not planes_ok:
        family = "tiles64"
    else:
        family = "planes"
    tail = attention_tail_rows(Sq, mask_mode, dense)
    nblk = Sq // ATTN_QB if tail else cdiv(Sq, ATTN_QB)
    pairs = H * B
    nW = nblk if pairs * nblk <= cus else max(1, min((nblk + 1) // 2 if mask_mode else nblk, cus // pairs))
    return family, tail, nW


# ---- the cases.  B = H = 0 with `persistent` set: the pair count is derived from the device (attention_fwd_case_resolve)
AttnFwdCase = collections.namedtuple(
    "AttnFwdCase", "hd prec Sq Sk B H Cq Ck mask dense table ws knobs layout wide ld_extra kind outputs ek_extra persistent")
ATTN_LAYOUTS = ("contig", "fused", "batch_first", "head2")
ATTN_KINDS = ("plain", "peaked", "late_max", "flat", "shifted")
ATTN_OUTPUTS = ("none", "lse", "lse+logits")
ATTN_SQ = (1, 33, 127, 128, 129, 257, 258, 259)
ATTN_SK = (1, 31, 32, 33, 63, 65, 97, 130, 257)
ATTN_CHANNELS = ((4, 1), (1, 4), (4, 4), (2, 1), (3, 2))
ATTN_DEFAULT_CUS = 256


def attention_fwd_case_id(c):
    return (f"hd{c.hd}-p{c.prec}-s{c.Sq}.{c.Sk}-b{c.B}h{c.H}-c{c.Cq}.{c.Ck}-m{c.mask}d{int(c.dense)}t{int(c.table)}-w{c.ws}k{c.knobs}-"
            f"{c.layout}{'+wide' if c.wide else ''}-ld{c.ld_extra}-{c.kind}-{c.outputs}-e{c.ek_extra}" + (f"-{c.persistent}" if c.persistent else ""))


def attention_fwd_case_resolve(c, cus=ATTN_DEFAULT_CUS):
    """A persistent case with its (batch, head) pairs for a device of `cus` CUs: "one": one pair more than CUs (nW = 1, one
    workgroup walks every block); "snake": cus // 2 pairs (pairs * blocks > cus >= 2 pairs: 1 < nW < blocks)."""
    if not c.persistent:
        return c
    pairs = cus + 1 if c.persistent == "one" else max(cus // 2, 1)
    H = 2 if pairs % 2 == 0 else 1
    return c._replace(B=pairs // H, H=H)


def attention_fwd_case_route(c, cus=ATTN_DEFAULT_CUS):
    c = attention_fwd_case_resolve(c, cus)
    Ek = -(-c.Sk // c.Ck) + c.ek_extra
    return attention_fwd_route(c.hd, c.prec, c.Cq, c.Ck, c.table, c.Sq, c.mask, c.dense, c.ws, c.knobs, cus, c.B, c.H, Sk=c.Sk,
                               rel_rows=-(-c.Sq // c.Cq) + Ek - 1)


def _attention_fwd_table():
    def ac(hd, prec, Sq, Sk, mask=0, dense=False, B=2, H=3, Cq=1, Ck=1, table=True, ws="none", knobs=0, layout="contig", wide=False,
           ld_extra=0, kind="plain", outputs="lse", ek_extra=0, persistent=""):
        if ws == "query" and prec in (2, 3):
            knobs |= ATTN_KNOB_FWD3_ALL           # the size query answers for the single-term modes only under this knob
        if prec == 0 and outputs == "lse+logits":
            outputs = "lse"                       # (kept logits are refused with precision 0)
        return AttnFwdCase(hd, prec, Sq, Sk, B, H, Cq, Ck, mask, dense, table, ws, knobs, layout, wide, ld_extra, kind, outputs, ek_extra,
                           persistent)
    # (Sq, Sk, mask, dense): every ragged length, mask and mask combination once per family
    slots = [(1, 1, 0, False), (33, 31, 0, False), (127, 32, 1, False), (128, 33, 2, False), (129, 97, 0, True), (257, 65, 1, False),
             (258, 130, 2, False), (259, 257, 0, False), (33, 63, 1, False), (129, 130, 1, True), (129, 129, 2, False),
             (257, 130, 2, False), (258, 97, 1, False)]
    insts = {"exact": [(hd, 0, None) for hd in (16, 32, 64)],
             "tiles64": [(hd, p, u) for u in (True, False) for p in (1, 2, 3) for hd in (16, 32, 64)],
             "planes": [(hd, p, True) for p in (1, 2, 3) for hd in (32, 64)]}
    cases = []
    for fam in ATTN_FAMILIES:
        n = max(len(slots), len(insts[fam]))
        general = 0
        for i in range(n):
            Sq, Sk, mask, dense = slots[i % len(slots)]
            hd, prec, unit = insts[fam][i % len(insts[fam])]
            Cq, Ck = 1, 1
            if fam == "exact" and i % 2:
                unit = False
            if unit is False:
                Cq, Ck = ATTN_CHANNELS[general % len(ATTN_CHANNELS)]
                general += 1
            layout = ATTN_LAYOUTS[i % 4]
            if (Sq, Sk) == (129, 129):
                layout = "fused"                 # q, k and v in ONE [S,B,3d] buffer
            cases.append(ac(hd, prec, Sq, Sk, mask, dense, H=4 if i % 3 == 0 else 3, Cq=Cq, Ck=Ck,
                            table=True if fam == "planes" else i % 4 != 3, ws="query" if fam == "planes" else "none", layout=layout,
                            wide=i % 2 == 1, ld_extra=32 * (i // 2 % 2), kind=ATTN_KINDS[i % 5], outputs=ATTN_OUTPUTS[i % 3],
                            ek_extra=3 if i == 6 else 0))
    # the one-row tail kernel: every head dim behind the 64-key tiles, 32 / 64 behind the planes; Sk below its 512 / G key groups
    for j, (hd, ws) in enumerate([(16, "none"), (32, "none"), (64, "none"), (32, "query"), (64, "query")]):
        cases.append(ac(hd, 1 + j % 3, (257, 258)[j % 2], (5, 257, 130)[j % 3], ws=ws, kind=ATTN_KINDS[j % 5], outputs="lse+logits",
                        layout=ATTN_LAYOUTS[j % 4], wide=j % 2 == 0, ld_extra=32 * (j % 2)))
    cases.append(ac(64, 2, 385, 5, ws="none", outputs="lse+logits", kind="late_max"))
    # causal, several channels per query event, ragged Sq: the kernels keep the ragged block last there (rel_attention_fwd2.hip:100)
    cases.append(ac(32, 1, 161, 161, 1, Cq=4, Ck=4, outputs="lse+logits", layout="fused"))
    cases.append(ac(32, 0, 161, 161, 1, Cq=2, Ck=1))
    # a workspace without a table: the 64-key tiles
    cases.append(ac(32, 1, 129, 65, 0, table=False, ws="given", outputs="lse+logits"))
    # a workspace handed over with a single-term mode and no knob: the planes ("a caller that hands one over anyway")
    cases.append(ac(64, 2, 130, 97, 1, ws="given", outputs="lse+logits", kind="peaked"))
    # the persistent schedule: at least three query blocks under both masks, pairs from the CU count
    for fam_ws, hd in (("none", 16), ("query", 32)):
        for how in ("one", "snake"):
            for mask in (1, 2):
                cases.append(ac(hd, 1 if how == "one" else 2, 257, 257, mask, B=0, H=0, ws=fam_ws, persistent=how,
                                outputs="lse+logits" if (how, mask) == ("snake", 1) else "lse", kind="plain" if mask == 1 else "late_max"))
    return cases


ATTENTION_FWD_CASES = _attention_fwd_table()
ATTENTION_FWD_ENTRY_CASES = [c for c in ATTENTION_FWD_CASES if not c.persistent and c.layout in ("contig", "fused", "batch_first")
                             and not c.wide and not c.ld_extra and c.ws != "given" and c.outputs == "lse+logits"][:6]


def _attention_fwd_features(c, cus):
    family, tail, nW = attention_fwd_case_route(c, cus)
    r = attention_fwd_case_resolve(c, cus)
    unit = c.Cq == 1 and c.Ck == 1
    f = {f"{family}: Sq {c.Sq}", f"{family}: Sk {c.Sk}", f"{family}: mask {c.mask}", f"{family}: layout {c.layout}",
         f"{family}: kind {c.kind}", f"{family}: outputs {c.outputs}", f"{family}: table {int(c.table)}",
         f"pairs % 8 {'==' if r.B * r.H % 8 == 0 else '!='} 0"}
    f.add({"exact": f"inst exact hd{c.hd}", "tiles64": f"inst tiles64 hd{c.hd} p{c.prec} {'unit' if unit else 'general'}",
           "planes": f"inst planes hd{c.hd} p{c.prec}"}[family])
    if tail:
        f.add(f"inst tail hd{c.hd} behind {family}")
        if c.Sk < 512 // (c.hd // 4):
            f.add("tail: Sk below the key groups")
    if c.Sq in (257, 258) and c.mask and not tail:
        f.add(f"{family}: Sq {c.Sq} masked, no tail")
    if c.dense:
        f.add(f"{family}: dense mask")
        if c.mask == 1:
            f.add(f"{family}: dense mask + causal")
    if c.mask == 1 and c.Sk != c.Sq:
        f.add(f"{family}: causal Sk {'<' if c.Sk < c.Sq else '>'} Sq")
    if c.mask == 2 and c.Sq > c.Sk:
        f.add(f"{family}: anti-causal Sq > Sk")
    if not unit:
        f.add(f"{family}: channels {c.Cq}.{c.Ck}")
    if c.mask == 1 and c.Cq != 1 and c.Sq % ATTN_QB:
        f.add(f"{family}: causal Cq != 1 ragged")
    if c.ek_extra:
        f.add(f"{family}: Ek above the key events")
    if c.wide:
        f.add(f"{family}: out in a wider buffer")
    if c.outputs == "lse+logits":
        f.add(f"{family}: logits_ld +{c.ld_extra}")
    if c.persistent and c.Sq > 2 * ATTN_QB:
        pairs, blocks = r.B * r.H, -(-c.Sq // ATTN_QB)
        if pairs > cus and nW == 1:
            f.add(f"{family}: persistent one mask {c.mask}")
        if pairs * blocks > cus >= 2 * pairs and 1 < nW < blocks:
            f.add(f"{family}: persistent snake mask {c.mask}")
    f.add(f"route: workspace {c.ws} p{c.prec} knobs {c.knobs} table {int(c.table)} -> {family}")
    return f


def attention_fwd_requirements():
    req = [f"inst exact hd{hd}" for hd in (16, 32, 64)]
    req += [f"inst tiles64 hd{hd} p{p} {u}" for hd in (16, 32, 64) for p in (1, 2, 3) for u in ("unit", "general")]
    req += [f"inst planes hd{hd} p{p}" for hd in (32, 64) for p in (1, 2, 3)]
    req += [f"inst tail hd{hd} behind tiles64" for hd in (16, 32, 64)] + [f"inst tail hd{hd} behind planes" for hd in (32, 64)]
    req += ["tail: Sk below the key groups", "pairs % 8 == 0", "pairs % 8 != 0"]
    req += ["route: workspace none p1 knobs 0 table 1 -> tiles64", "route: workspace query p1 knobs 0 table 1 -> planes",
            "route: workspace query p2 knobs 2 table 1 -> planes", "route: workspace query p3 knobs 2 table 1 -> planes",
            "route: workspace given p1 knobs 0 table 0 -> tiles64", "route: workspace given p2 knobs 0 table 1 -> planes"]
    for fam in ATTN_FAMILIES:
        req += [f"{fam}: Sq {s}" for s in ATTN_SQ] + [f"{fam}: Sk {s}" for s in ATTN_SK] + [f"{fam}: mask {m}" for m in (0, 1, 2)]
        req += [f"{fam}: Sq {s} masked, no tail" for s in (257, 258)]
        req += [f"{fam}: dense mask", f"{fam}: dense mask + causal", f"{fam}: causal Sk < Sq", f"{fam}: causal Sk > Sq",
                f"{fam}: anti-causal Sq > Sk", f"{fam}: Ek above the key events", f"{fam}: out in a wider buffer", f"{fam}: table 1"]
        req += [f"{fam}: layout {l}" for l in ATTN_LAYOUTS] + [f"{fam}: kind {k}" for k in ATTN_KINDS]
        req += [f"{fam}: outputs {o}" for o in ATTN_OUTPUTS if fam != "exact" or o != "lse+logits"]
        if fam != "planes":
            req += [f"{fam}: channels {a}.{b}" for a, b in ATTN_CHANNELS] + [f"{fam}: causal Cq != 1 ragged", f"{fam}: table 0"]
        if fam != "exact":
            req += [f"{fam}: logits_ld +0", f"{fam}: logits_ld +32"]
            req += [f"{fam}: persistent {how} mask {m}" for how in ("one", "snake") for m in (1, 2)]
    return req


def attention_fwd_coverage_gaps(cases, cus=ATTN_DEFAULT_CUS):
    """The requirements of the case table (every instantiation; per family the ragged lengths, masks, channel layouts,
    buffer layouts, data kinds, requested outputs and persistent schedules; the routes as the code offers them) that no
    case of `cases` covers."""
    have = set()
    for c in cases:
        have |= _attention_fwd_features(c, cus)
    return [r for r in attention_fwd_requirements() if r not in have]


AttnData = collections.namedtuple("AttnData", "q k v rel dense scale Ek rel_rows empty_rows")


def attention_fwd_case_data(c):
    """The inputs of a (resolved) case, seeded from its id: q [Sq,B,H,hd], k / v [Sk,B,H,hd], the table, the dense mask, scale,
    Ek, rel_rows, and `empty_rows`: the query rows the case designs to be empty (anti-causal rows beyond the last key; the
    all -inf row of a dense mask).  Kinds: plain: randn, table x 0.5; peaked: q x 6; late_max: the logits grow with the key
    index, so the running maximum moves in every tile and arrives in the last; flat: k = 0 and table = 0 (uniform weights,
    out = mean of v, lse = ln(allowed count)); shifted: every logit about -80 (natural units)."""
    import zlib
    assert c.B > 0 and c.H > 0, "resolve a persistent case first"
    gen = torch.Generator().manual_seed(zlib.crc32(attention_fwd_case_id(c._replace(B=0, H=0) if c.persistent else c).encode()))
    rn = lambda *s: torch.randn(*s, generator=gen)
    Sq, Sk, B, H, hd = c.Sq, c.Sk, c.B, c.H, c.hd
    scale = float(np.float32(1.0 / math.sqrt(hd)))
    Ek = -(-Sk // c.Ck) + c.ek_extra
    rel_rows = -(-Sq // c.Cq) + Ek - 1
    q, k, v = rn(Sq, B, H, hd), rn(Sk, B, H, hd), rn(Sk, B, H, hd)
    rel = rn(H, rel_rows, hd) * 0.5 if c.table else None
    if c.kind == "peaked":
        q = q * 6.0
    elif c.kind == "late_max":
        q = q.abs()
        k = k * 0.2 + 2.0 * (torch.arange(Sk, dtype=torch.float32)[:, None, None, None] + 1.0) / Sk
    elif c.kind == "flat":
        k = torch.zeros_like(k)
        rel = None if rel is None else torch.zeros_like(rel)
    elif c.kind == "shifted":
        u = torch.nn.functional.normalize(rn(1, B, H, hd), dim=-1)
        q, k = 4.0 * u + 0.3 * q, -(20.0 / scale) * u + k
    else:
        assert c.kind == "plain", c.kind
    dense, empty = None, set()
    if c.mask == 2:
        empty |= set(range(Sk, Sq))
    if c.dense:
        assert Sk > 64 and Sq > 66 and c.mask in (0, 1)
        dense = rn(Sq, Sk)
        dense[torch.rand(Sq, Sk, generator=gen) < 0.15] = float("-inf")
        rows = torch.arange(Sq)
        cols = rows.clamp(max=Sk - 1)
        dense[rows, cols] = dense[rows, cols].nan_to_num(neginf=0.5)     # every row keeps a live pair both masks allow ...
        r_all, r_late = Sq // 2, Sq - 1
        dense[r_all] = float("-inf")                                     # ... but this one: an empty row
        dense[r_late, :64] = float("-inf")                               # the online softmax sees two whole tiles of -inf first
        empty.add(r_all)
    return AttnData(q, k, v, rel, dense, scale, Ek, rel_rows, sorted(empty))


AttnRefs = collections.namedtuple("AttnRefs", "spec f32 model yard tail empty")


def _attn_finite(t):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


def attention_fwd_refs(c, d, tail, models=True):
    """spec, float32 yardstick, the mode's model (None for precision 0) and the yardstick of the hold: per element the
    worse of the float32 evaluation and the model on the tile rows of precisions 1 .. 3, the float32 evaluation alone for
    precision 0 and for the last `tail` query rows (the one-row kernel is exact fp32); `empty`: [B,H,Sq] rows the spec finds
    empty."""
    a = (d.q, d.k, d.v, d.rel, c.H, c.Cq, c.Ck, d.Ek, c.mask, d.dense, d.scale)
    spec, f32 = attention_fwd_spec(*a), attention_fwd_f32(*a)
    f32 = AttnFwd(f32.out.double(), f32.lse.double(), f32.logits2.double(), f32.allowed)
    assert bool(torch.isfinite(f32.out).all()) and bool(torch.isfinite(f32.lse).all()), "the float32 yardstick is not finite on this data"
    model, yard = None, f32
    if c.prec and models:
        model = attention_fwd_model(*a, c.prec)
        yo = larger_error(f32.out, model.out, spec.out)
        yl = larger_error(f32.lse, model.lse, spec.lse)
        yg = larger_error(_attn_finite(f32.logits2), _attn_finite(model.logits2), _attn_finite(spec.logits2))
        if tail:
            yo[:, :, -tail:], yl[:, :, -tail:], yg[:, :, -tail:] = f32.out[:, :, -tail:], f32.lse[:, :, -tail:], _attn_finite(f32.logits2[:, :, -tail:])
        yard = AttnFwd(yo, yl, yg, spec.allowed)
    return AttnRefs(spec, f32, model, yard, tail, spec.lse == ATTN_EMPTY_LSE)


@functools.lru_cache(maxsize=2)
def attention_fwd_case_refs(c, cus=ATTN_DEFAULT_CUS):
    """(resolved case, data, refs) of a case on a device of `cus` CUs; computed once per case."""
    r = attention_fwd_case_resolve(c, cus)
    d = attention_fwd_case_data(r)
    return r, d, attention_fwd_refs(r, d, attention_fwd_case_route(c, cus)[1])


def attention_fwd_hold(got, refs, what, yard=None, margin=ROW_OPS_MARGIN):
    """The hold of the attention forward: compare_rows with the project's margin and floor on
      out     rows = the hd values of one (batch, head, query); an empty row is 0 exactly;
      lse     (got.lse is not None) the vector without the empty rows, which equal ATTN_EMPTY_LSE exactly;
      logits  (got.logits2 is not None: [B,H,Sq,>= Sk]) per query row over the allowed columns: disallowed entries and the
              columns from Sk on are unspecified (0 on both sides), a -inf entry must be -inf exactly (then 0).
    The tile rows and the last refs.tail query rows (the one-row kernel's, float32 yardstick) are blocks of their own, as in
    linear_hold.  Returns {"out" | "lse" | "logits" | "tail out" | ...: RowCheck}; raises AssertionError at the first failure."""
    spec, yard = refs.spec, yard or refs.yard
    Sq, Sk = spec.logits2.shape[-2:]
    out = torch.as_tensor(got.out).detach().cpu()
    assert out.shape == spec.out.shape, f"{what}: out {tuple(out.shape)} against {tuple(spec.out.shape)}"
    lse = None if got.lse is None else torch.as_tensor(got.lse).detach().cpu()
    lg = None if got.logits2 is None else torch.as_tensor(got.logits2).detach().cpu()[..., :Sk].double()
    assert lse is None or lse.shape == spec.lse.shape
    assert lg is None or lg.shape == spec.logits2.shape, f"{what}: logits {tuple(lg.shape)} against {tuple(spec.logits2.shape)}"
    checks = {}
    for name, rows in (("", slice(0, Sq - refs.tail)), ("tail ", slice(Sq - refs.tail, Sq))):
        if rows.start == rows.stop:
            continue
        empty = refs.empty[:, :, rows]
        assert bool((out[:, :, rows][empty] == 0).all()), f"{what}: an empty row's out is not 0"
        checks[name + "out"] = compare_rows(out[:, :, rows], spec.out[:, :, rows], yard.out[:, :, rows], f"{what} {name}out", margin)
        if lse is not None:
            assert bool((lse[:, :, rows][empty] == ATTN_EMPTY_LSE).all()), f"{what}: an empty row's lse is not 1e30"
            if not bool(empty.all()):
                checks[name + "lse"] = compare_rows(lse[:, :, rows][~empty], spec.lse[:, :, rows][~empty], yard.lse[:, :, rows][~empty],
                                                    f"{what} {name}lse", margin)
        if lg is not None:
            sl = spec.logits2[:, :, rows]
            allowed = spec.allowed[rows].expand_as(sl)
            ninf = allowed & (sl == float("-inf"))
            assert bool((lg[:, :, rows][ninf] == float("-inf")).all()), f"{what}: a -inf logit is not -inf"
            keep, zero = allowed & ~ninf, torch.zeros_like(sl)
            checks[name + "logits"] = compare_rows(torch.where(keep, lg[:, :, rows], zero), torch.where(keep, sl, zero),
                                                   torch.where(keep, _attn_finite(yard.logits2[:, :, rows]), zero),
                                                   f"{what} {name}logits", margin)
    return checks


# ---------------------------------------------------------------------------------------------------------------------
# Float64 specification, float32 yardstick, split-product model, route mirror and case table of the relative-attention
# BACKWARD (isi_rel_attention_bwd_f32: csrc/rel_attention_bwd_f32.hip, planned by csrc/rel_attention_run.cpp), on the
# helpers of the forward's block above.  The operation, as the header of rel_attention_bwd_f32.hip states it, is a function
# of the GIVEN float32 tensors q, k, v, e, dense mask, scale, dO, out, lse and (kept-logits calls) logits -- not the
# derivative of some forward run:
#     P = exp(logit - lse)        logit recomputed as in the forward, or logits_given (base 2) for the SAVED kernels
#     D_i = sum_d dO[i,d] out[i,d]         dS = P o (dO V^T - D) * scale
#     dV = P^T dO    dK = dS^T Q    G[i,r] = sum_{j: r(i,j) = r} dS[i,j]    dQ = dS K + G E    dE = G^T Q
# A row whose lse is ATTN_EMPTY_LSE, a pair the mask leaves out and a pair whose logit is -inf contribute exactly 0 (not
# NaN); d_rel rows no allowed pair selects are exactly 0.
# Tensors here: q / dO / out [Sq,B,H,hd], k / v [Sk,B,H,hd], lse [B,H,Sq], logits [B,H,Sq,>= Sk]; results dq [B,H,Sq,hd],
# dk / dv [B,H,Sk,hd], d_rel [H,rel_rows,hd] (None without a table).
# tests/test_attention_bwd_host.py holds the spec to float64 autograd and shows what the hold rejects;
# tests/test_attention_bwd_gpu.py holds every kernel route to it.
ATTN_KNOB_FULL_ZERO, ATTN_KNOB_NO_G_FROM_KV, ATTN_KNOB_NO_GEMM = 4, 8, 16      # bits of `knobs`, as in tests/attention_plan_tracer.cpp
ATTN_BWD_KNOBS = {ATTN_KNOB_FULL_ZERO: ("ISI_ATTN_FULL_ZERO", 1), ATTN_KNOB_NO_G_FROM_KV: ("ISI_ATTN_G_FROM_KV", 0),
                  ATTN_KNOB_NO_GEMM: ("ISI_NO_GEMM_KERNEL", 1)}               # bit -> (switch, the value the bit sets)
ATTN_G_MARGIN = 160                                # kMargin of rel_attention_bwd_f32.hip: columns zeroed on either side of a row's band of G
ATTN_BWD_FAMILIES = ("exact", "split", "saved")    # the exact-fp32 pair | the split pair recomputing its logits | reading kept ones
AttnBwd = collections.namedtuple("AttnBwd", "dq dk dv d_rel")
AttnBwdRoute = collections.namedtuple(
    "AttnBwdRoute", "has_e split one saved unit gemm_path band_only g_from_kv tail_q tail_k rho Rp band g_off g_len")


def _attention_bwd_eval(dtype, q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, d_out, out, lse, logits=None, no_D=False,
                        no_scale=False, scale_twice_ge=False, rel_shift=0, swap_c_in_g=False, strict_causal=False, drop_last_key=False,
                        g_drop_last_query=False, de_drop_query=None, de_drop_last_batch=False, junk_outside_rho=None):
    """The operation in `dtype`; every keyword behind `logits` is a mutant of the host tests (off: the operation as specified):
    no_D: D left out of dS; no_scale: dS without `scale`; scale_twice_ge: the G E share of dQ scaled again; rel_shift: r(i,j)
    off by that much; swap_c_in_g: Cq and Ck exchanged in G's index; strict_causal: the diagonal excluded; drop_last_key: the
    last key of a ragged 32-key tile left out of dK / dV; g_drop_last_query: the last query's row of G left 0 (its dQ still
    has dS K); de_drop_query: that query left out of dE; de_drop_last_batch: the last batch item left out of dE;
    junk_outside_rho = (lo, n): the d_rel rows outside [lo, lo + n) not zeroed (they hold 1)."""
    hq, hk, hv, hdo, ho = (_attn_heads(t, H).to(dtype) for t in (q, k, v, d_out, out))
    B, _, Sq, _ = hq.shape
    Sk = hk.shape[2]
    lse = torch.as_tensor(lse).detach().cpu()
    allowed = attention_allowed(Sq, Sk, mask_mode, strict=strict_causal)
    e = None if rel is None else torch.as_tensor(rel).detach().cpu().to(dtype)

    def index(cq, ck):
        idx = attention_rel_index(Sq, Sk, cq, ck, Ek) + rel_shift
        if rel_shift or (cq, ck) != (Cq, Ck):
            idx = idx.clamp(0, e.shape[1] - 1)
        assert int(idx.min()) >= 0 and int(idx.max()) < e.shape[1], "the table must cover every (query, key) pair"
        return idx.expand(B, H, Sq, Sk)

    if logits is None:
        s = hq @ hk.transpose(-1, -2)
        if e is not None:
            s = s + torch.einsum("bhid,hrd->bhir", hq, e).gather(3, index(Cq, Ck))
        l2 = s * (scale * ATTN_LOG2E)
        if dense_mask is not None:
            l2 = l2 + torch.as_tensor(dense_mask).detach().cpu().to(dtype) * ATTN_LOG2E
    else:
        l2 = torch.as_tensor(logits).detach().cpu()[..., :Sk].to(dtype)
    empty = lse == ATTN_EMPTY_LSE
    zero = torch.zeros((), dtype=dtype)
    live = allowed & (l2 > float("-inf")) & ~empty[..., None]        # (a NaN of a kept-logits buffer compares false: never read)
    lse2 = torch.where(empty, zero, lse.to(dtype) * ATTN_LOG2E)[..., None]
    P = torch.where(live, torch.exp2(torch.where(live, l2, zero) - lse2), zero)
    D = (hdo * ho).sum(-1, keepdim=True)
    dS = P * (hdo @ hv.transpose(-1, -2) - (0.0 if no_D else D))
    if not no_scale:
        dS = dS * scale
    Pk, dSk = P, dS
    if drop_last_key and Sk % 32:
        Pk, dSk = P.clone(), dS.clone()
        Pk[..., Sk - 1] = 0
        dSk[..., Sk - 1] = 0
    dV, dK, dQ, dE = Pk.transpose(-1, -2) @ hdo, dSk.transpose(-1, -2) @ hq, dS @ hk, None
    if e is not None:
        R = e.shape[1]
        G = torch.zeros(B, H, Sq, R, dtype=dtype).scatter_add_(3, index(*((Ck, Cq) if swap_c_in_g else (Cq, Ck))), dS)
        if g_drop_last_query:
            G[:, :, Sq - 1] = 0
        ge = torch.einsum("bhir,hrd->bhid", G, e)
        dQ = dQ + (ge * scale if scale_twice_ge else ge)
        Gd = G
        if de_drop_query is not None and de_drop_query < Sq:
            Gd = Gd.clone()
            Gd[:, :, de_drop_query] = 0
        if de_drop_last_batch:
            Gd = Gd.clone()
            Gd[B - 1] = 0
        dE = torch.einsum("bhir,bhid->hrd", Gd, hq)
        if junk_outside_rho is not None:
            lo, n = junk_outside_rho
            dE[:, :lo] = 1
            dE[:, lo + n:] = 1
    return AttnBwd(dQ, dK, dV, dE)


def attention_bwd_spec(q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, d_out, out, lse, logits=None):
    """The float64 specification: AttnBwd(dq, dk, dv, d_rel) of the given tensors (logits: the kept base-2 logits of a
    SAVED call, else None and they are recomputed)."""
    return _attention_bwd_eval(torch.float64, q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, d_out, out, lse, logits)


def attention_bwd_f32(q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, d_out, out, lse, logits=None, **mutant):
    """The same evaluation in float32 torch on the CPU: the yardstick (and what the host tests mutate)."""
    return _attention_bwd_eval(torch.float32, q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, d_out, out, lse, logits, **mutant)


def attention_bwd_model(q, k, v, rel, H, Cq, Ck, Ek, mask_mode, dense_mask, scale, d_out, out, lse, logits, precision, saved, drop=None,
                        tail_q=0, tail_k=0, g_from_kv=False, renorm_lse=False):
    """Float64 evaluation on the operands the split pair multiplies; its distance from the spec is the truncation the mode
    accepts by design.  Read from csrc/rel_attention_bwd_f32.hip (rel_attention_bwd_q_split_kernel /
    rel_attention_bwd_kv_split_kernel) and csrc/rel_attention_run.cpp:
      * precision 1 and 3 run the three-term kernels, precision 2 the single-term ones (run.cpp make_route: `r.one =
        g->precision == 2`; launch_bwd_split_hd): hi = rne_bf16(x), lo = rne_bf16(x - hi) (split_f4 / split2, csrc/split_bf16.h),
        terms `ISI_MFB(kl, qh); ISI_MFB(kh, qlo); ISI_MFB(kh, qh)` with the first two under `if constexpr (!ONE)`;
      * Q and dO are converted AS THEY ARE (q kernel lines 622-637: `split_f4(buf_load4(rq, oq), h0, l0)`; kv kernel's commit,
        lines 1139-1156), as are K and V (kv kernel lines 1044-1059; q kernel's commit, lines 691-716) and the table rows
        (`put_e`, lines 684-690 and 1116-1122): `scale` is NOT folded into an operand -- the float32 sum is multiplied by
        scale2 = scale * log2(e) afterwards (`sv[r] * sc2 - lse2`, lines 852-866 and 1319-1334) and the dense mask added in
        float32 as mask * log2(e);
      * S = Q K^T and the band product Q E^T: lines 806-848 and 1267-1312 (products "qk", "band");
      * with `saved` the logits are the given float32 values, no product (`sc2 = saved ? 1.f : scale2`, lines 797-803, 1261-1265);
      * P = exp2(logit2 - lse log2(e)) in float32; dP = dO V^T on converted operands (lines 870-879, 1361-1370: "dp"),
        dS = P (dP - D) scale in float32 with D = sum dO out in float32 (attn_dsum_kernel);
      * dV = P^T dO multiplies the converted float32 P (`split_acc16(sv, sh, sl)`, line 1339) with converted dO (lines
        1341-1357: "dv"); dK = dS^T Q and dQ = dS K the converted float32 dS with converted Q / K (lines 1407-1425: "dk";
        lines 886-905: "dq");
      * G holds the float32 dS; both products over it run three-term products under EVERY precision >= 1 (run.cpp line 328:
        `gemm_flags = r.split ? ISI_CONV_BF16X3 : 0`, also for precision 2): dQ += G E on gemm_split_f32 (split_mode 1) or
        the 1x1 convolution ("ge"), dE = G^T Q on conv_wgrad_batched_f32 ("de").  (The convolution ignores the flag for
        short contractions -- include/isi_hip.h, "K < 128" -- and is exact fp32 there: closer to the spec than this model.)
      * the one-row kernels (attn_bwd_tail_row / attn_bwd_tail_key, lines 1505-1627) are exact fp32 on recomputed logits: the
        last tail_q query rows of dS (their dQ = dS K and their rows of G) and the last tail_k keys (dK, dV; with g_from_kv
        their columns of G, line 1606) are the unconverted float64 values here.  A tail query's dQ still receives G E from
        the three-term product like every other row;
      * g_from_kv: the query-stationary kernel reads dS back from G (lines 776-794), the tail keys' exact columns included.
    `drop` = one of "qk" "band" "dp" "dv" "dk" "dq" "ge" "de": that product without its lo.hi term; renorm_lse: the given lse
    replaced by the log-sum-exp of the model's own logits -- host-test mutants."""
    assert precision in (1, 2, 3), precision
    pp = 2 if precision == 2 else 1
    hq, hk, hv, hdo, ho = (_attn_heads(t, H).float() for t in (q, k, v, d_out, out))
    B, _, Sq, _ = hq.shape
    Sk = hk.shape[2]
    lse = torch.as_tensor(lse).detach().cpu()
    T = lambda A, Bp, contract, name: _attn_terms(A, Bp, contract, "lo_hi" if drop == name else None)
    Qp, Kp, Vp, DOp = (_attn_pieces(t, pp) for t in (hq, hk, hv, hdo))
    allowed = attention_allowed(Sq, Sk, mask_mode)
    e = idx = None
    if rel is not None:
        e = torch.as_tensor(rel).detach().cpu().float()
        idx = attention_rel_index(Sq, Sk, Cq, Ck, Ek).expand(B, H, Sq, Sk)
        assert int(idx.min()) >= 0 and int(idx.max()) < e.shape[1]
    scale2 = float(np.float32(scale) * np.float32(ATTN_LOG2E))
    dm = None if dense_mask is None else torch.as_tensor(dense_mask).detach().cpu().double() * ATTN_LOG2E

    def logits2(Qx, Kx, Ex):
        s = T(Kx, Qx, lambda a, b: b @ a.transpose(-1, -2), "qk")
        if e is not None:
            s = s + T(Ex, Qx, lambda a, b: torch.einsum("bhid,hrd->bhir", b, a), "band").gather(3, idx)
        s = s * scale2
        return s if dm is None else s + dm

    empty = lse == ATTN_EMPTY_LSE
    zero = torch.zeros((), dtype=torch.float64)
    D = (hdo.double() * ho.double()).sum(-1, keepdim=True)

    def p_ds(l2, dP):
        live = allowed & (l2 > float("-inf"))
        none, given = empty, lse.double() * ATTN_LOG2E
        if renorm_lse:
            none = ~live.any(-1)
            given = torch.log2(torch.where(live, torch.exp2(torch.where(live, l2, zero)), zero).sum(-1).clamp(min=2.0 ** -1000))
        live = live & ~none[..., None]
        lse2 = torch.where(none, zero, given)[..., None]
        P = torch.where(live, torch.exp2(torch.where(live, l2, zero) - lse2), zero)
        return P, P * (dP - D) * scale

    l2 = (torch.as_tensor(logits).detach().cpu()[..., :Sk].double() if saved
          else logits2(Qp, Kp, None if e is None else _attn_pieces(e, pp)))
    P, dS = p_ds(l2, T(Vp, DOp, lambda a, b: b @ a.transpose(-1, -2), "dp"))
    dS_g = dS
    if tail_q or tail_k:
        one = lambda t: (t.double(),)
        Px, dSx = p_ds(logits2(one(hq), one(hk), None if e is None else one(e)), hdo.double() @ hv.double().transpose(-1, -2))
        dS_g = dS.clone()
        if tail_q:
            dS_g[:, :, Sq - tail_q:] = dSx[:, :, Sq - tail_q:]
        if tail_k and g_from_kv:
            dS_g[..., Sk - tail_k:] = dSx[..., Sk - tail_k:]
    Pp, dSp = _attn_pieces(P.float(), pp), _attn_pieces(dS.float(), pp)
    dV = T(DOp, Pp, lambda a, b: b.transpose(-1, -2) @ a, "dv")
    dK = T(Qp, dSp, lambda a, b: b.transpose(-1, -2) @ a, "dk")
    dQ = T(Kp, _attn_pieces(dS_g.float(), pp) if g_from_kv else dSp, lambda a, b: b @ a, "dq")
    if tail_k:
        dV[:, :, Sk - tail_k:] = (Px.transpose(-1, -2) @ hdo.double())[:, :, Sk - tail_k:]
        dK[:, :, Sk - tail_k:] = (dSx.transpose(-1, -2) @ hq.double())[:, :, Sk - tail_k:]
    if tail_q:
        dQ[:, :, Sq - tail_q:] = (dSx @ hk.double())[:, :, Sq - tail_q:]
    dE = None
    if e is not None:
        G = torch.zeros(B, H, Sq, e.shape[1], dtype=torch.float64).scatter_add_(3, idx, dS_g.float().double())
        Gp, E1, Q1 = _attn_pieces(G.float(), 1), _attn_pieces(e, 1), _attn_pieces(hq, 1)
        dQ = dQ + T(E1, Gp, lambda a, b: torch.einsum("bhir,hrd->bhid", b, a), "ge")
        dE = T(Q1, Gp, lambda a, b: torch.einsum("bhir,bhid->hrd", b, a), "de")
    return AttnBwd(dQ, dK, dV, dE)


def gemm_split_applicable(M, N, K, split_mode=1):
    """gemm_split_applicable of csrc/gemm_split_f32.hip"""
    return split_mode in (1, 3) and K % 32 == 0 and K >= 128 and N > 32 and M >= 256


def attention_bwd_route(hd, precision, Cq, Ck, table, Sq, Sk, B, H, mask_mode, dense, logits, q_uniform, knobs, Ek, rel_rows,
                        gemm_ok=None):
    """Restatement of rho_range, g_band, carve (G's place), make_route and attention_tail_rows of csrc/rel_attention_run.cpp
    for an accepted backward call.  logits: kept logits are handed over; q_uniform: q_ss == B * q_sb; knobs: bits
    ATTN_KNOB_FULL_ZERO | ATTN_KNOB_NO_G_FROM_KV | ATTN_KNOB_NO_GEMM; gemm_ok: the answer of gemm_split_applicable(Sq B, hd,
    Rp, 1), asked here when None.  rho = (lo, n): the table rows G covers; Rp: n padded to the 32-row K chunk; band =
    (lo_slope, lo_base, hi_slope, hi_base): query i of a unit-channel call is non-zero in columns [lo_slope i + lo_base,
    hi_slope i + hi_base] of G; g_off, g_len: G's place in the workspace in floats, laid out [H][Sq][B][Rp]."""
    R = rel_rows if table else 0
    has_e = R > 0
    lo, n = 0, R
    if has_e and Cq == Ck and not dense:
        if mask_mode == 1:
            lo = min(max(Ek - 1, 0), R - 1)
            n = R - lo
        if mask_mode == 2:
            n = max(1, min(R, Ek))
    Rp = -(-max(n, 1) // 32) * 32
    split, one, unit = precision >= 1, precision == 2, Cq == 1 and Ck == 1
    saved = split and bool(logits)
    if gemm_ok is None:
        gemm_ok = gemm_split_applicable(Sq * B, hd, Rp, 1)
    gemm_path = bool(has_e and split and q_uniform and gemm_ok and not knobs & ATTN_KNOB_NO_GEMM)
    band_only = bool(unit and gemm_path and not knobs & ATTN_KNOB_FULL_ZERO)
    g_from_kv = bool(band_only and saved and not knobs & ATTN_KNOB_NO_G_FROM_KV)
    tail_q = attention_tail_rows(Sq, mask_mode, dense) if split and (not has_e or Ck == 1) else 0
    tail_k = attention_tail_rows(Sk, mask_mode, dense) if split else 0
    top, bot = Ek - 1 - lo, Ek - Sk - lo
    band = (0 if mask_mode == 1 else 1, top if mask_mode == 1 else bot, 0 if mask_mode == 2 else 1, top)
    return AttnBwdRoute(has_e, split, one, saved, unit, gemm_path, band_only, g_from_kv, tail_q, tail_k, (lo, n), Rp, band,
                        -(-(B * H * Sq) // 64) * 64, H * B * Sq * Rp if has_e else 0)


def attention_bwd_launches(r):
    """launches per launcher of an accepted call on route r, as tests/attention_plan_tracer.cpp counts them"""
    want = {"attn_dsum": 1}
    if r.split:
        want["attn_bwd_split"] = 2 if r.g_from_kv else 1
        if r.tail_q or r.tail_k:
            want["attn_bwd_tails"] = 1
    else:
        want["attn_bwd_exact"] = 1
    if r.has_e:
        want["attn_zero_g_margins" if r.band_only else "attn_zero_g"] = 1
        want["gemm_split" if r.gemm_path else "conv2d_batched"] = 1
        want.update(pack_rel_T=1, conv_wgrad_batched=1, unpack_drel=1)
    return want


# ---- the cases.  B = H = 0 with `persistent` set: the pair count is derived from the device (attention_fwd_case_resolve)
AttnBwdCase = collections.namedtuple(
    "AttnBwdCase", "hd prec Sq Sk B H Cq Ck mask dense table saved knobs layout wide ld_extra kind ek_extra persistent scale_mul")
ATTN_BWD_KINDS = ("plain", "peaked", "flat", "shifted")
ATTN_BWD_TAIL_SIZES = (257, 258, 385)


def attention_bwd_case_id(c):
    return (f"hd{c.hd}-p{c.prec}{'s' if c.saved else ''}-s{c.Sq}.{c.Sk}-b{c.B}h{c.H}-c{c.Cq}.{c.Ck}-m{c.mask}d{int(c.dense)}t{int(c.table)}-"
            f"k{c.knobs}-{c.layout}{'+wide' if c.wide else ''}-ld{c.ld_extra}-{c.kind}-e{c.ek_extra}-x{c.scale_mul:g}"
            + (f"-{c.persistent}" if c.persistent else ""))


def attention_bwd_case_resolve(c, cus=ATTN_DEFAULT_CUS):
    """A persistent case with the forward's device-derived pair count: "one": cus + 1 (batch, head) pairs, "snake": cus // 2."""
    if not c.persistent:
        return c
    r = attention_fwd_case_resolve(_attention_bwd_fwd_case(c), cus)
    return c._replace(B=r.B, H=r.H)


def _attention_bwd_fwd_case(c):
    """the forward case whose data (attention_fwd_case_data) the backward case differentiates"""
    return AttnFwdCase(c.hd, c.prec, c.Sq, c.Sk, c.B, c.H, c.Cq, c.Ck, c.mask, c.dense, c.table, "none", 0, c.layout, c.wide, c.ld_extra,
                       c.kind, "lse", c.ek_extra, c.persistent)


def attention_bwd_case_route(c, cus=ATTN_DEFAULT_CUS, gemm_ok=None):
    c = attention_bwd_case_resolve(c, cus)
    Ek = -(-c.Sk // c.Ck) + c.ek_extra
    return attention_bwd_route(c.hd, c.prec, c.Cq, c.Ck, c.table, c.Sq, c.Sk, c.B, c.H, c.mask, c.dense, c.saved,
                               c.layout != "batch_first", c.knobs, Ek, -(-c.Sq // c.Cq) + Ek - 1, gemm_ok)


def attention_bwd_family(c):
    return "exact" if c.prec == 0 else "saved" if c.saved else "split"


def _attention_bwd_table():
    def bc(hd, prec, Sq, Sk, mask=0, dense=False, B=2, H=3, Cq=1, Ck=1, table=True, saved=False, knobs=0, layout="contig", wide=False,
           ld_extra=0, kind="plain", ek_extra=0, persistent="", scale_mul=1.0):
        return AttnBwdCase(hd, prec, Sq, Sk, B, H, Cq, Ck, mask, dense, table, bool(saved and prec), knobs, layout, wide,
                           ld_extra if saved and prec else 0, kind, ek_extra, persistent, scale_mul)
    # (Sq, Sk, mask, dense): every ragged length, mask and mask combination once per family, as in the forward's table
    slots = [(1, 1, 0, False), (33, 31, 0, False), (127, 32, 1, False), (128, 33, 2, False), (129, 97, 0, True), (257, 65, 1, False),
             (258, 130, 2, False), (259, 257, 0, False), (33, 63, 1, False), (129, 130, 1, True), (129, 129, 2, False),
             (257, 130, 2, False), (258, 97, 1, False)]
    insts = {"exact": [(hd, 0) for hd in (16, 32, 64)], "split": [(hd, p) for p in (1, 2, 3) for hd in (16, 32, 64)]}
    insts["saved"] = insts["split"]
    cases = []
    for fam in ATTN_BWD_FAMILIES:
        general = 0
        for i, (Sq, Sk, mask, dense) in enumerate(slots):
            hd, prec = insts[fam][i % len(insts[fam])]
            Cq, Ck = 1, 1
            if i % 2:
                Cq, Ck = ATTN_CHANNELS[general % len(ATTN_CHANNELS)]
                general += 1
            cases.append(bc(hd, prec, Sq, Sk, mask, dense, B=2 + i % 3, H=3 if i % 2 else 2, Cq=Cq, Ck=Ck, table=i % 4 != 3,
                            saved=fam == "saved", layout="fused" if (Sq, Sk) == (129, 129) else ATTN_LAYOUTS[i % 4], wide=i % 2 == 1,
                            ld_extra=32 * (i // 2 % 2), kind=ATTN_BWD_KINDS[i % 4], ek_extra=3 if i in (5, 6) else 0))
    # dQ += G E on the banded GEMM: head_dim 64, Sq B >= 256, Rp >= 128, one channel per event; every mask; the three
    # switches; kept logits with and without g_from_kv.  129 x 129 is the smallest such shape, 385 x 385 the smallest whose
    # G has elements further than kMargin from a row's band (and, unmasked, a one-row / one-key tail)
    for mask in (0, 1, 2):
        for j, (saved, knobs) in enumerate([(False, 0), (False, ATTN_KNOB_FULL_ZERO), (False, ATTN_KNOB_NO_GEMM), (True, 0),
                                            (True, ATTN_KNOB_NO_G_FROM_KV)]):
            cases.append(bc(64, 1 + (mask + j) % 3, 129, 129, mask, saved=saved, knobs=knobs, H=2, kind=ATTN_BWD_KINDS[(mask + j) % 4],
                            layout=("contig", "fused", "head2")[(mask + j) % 3]))
    for mask, saved, knobs in [(0, False, 0), (1, True, 0), (2, False, 0), (0, False, ATTN_KNOB_FULL_ZERO), (1, False, ATTN_KNOB_NO_GEMM),
                               (0, True, 0), (2, True, ATTN_KNOB_NO_G_FROM_KV)]:
        cases.append(bc(64, 1 if mask != 1 else 2, 385, 385, mask, saved=saved, knobs=knobs, H=2))
    # the same shapes where gemm_split_applicable declines: head_dim 32 and 16 (N > 32), Sq B < 256 (M >= 256), and q rows
    # that are no [Sq B, .] matrix (batch_first); 385 x 385 shows the full zero on the device
    cases += [bc(32, 1, 129, 129, 0), bc(16, 2, 129, 129, 1, saved=True), bc(32, 3, 385, 385, 0, H=2), bc(16, 1, 385, 385, 2, H=2, saved=True),
              bc(64, 1, 127, 127, 0, B=2), bc(64, 1, 129, 129, 0, layout="batch_first"), bc(64, 2, 385, 385, 1, H=2, layout="batch_first", saved=True)]
    # tails (unmasked, no dense mask, split pair): 257, 258 and 385 on either side, 259 a block again; Ck = 2 declines the
    # tail query; one side alone; without a table; kept logits with g_from_kv (the one-key kernel stores its column of G)
    cases += [bc(64, 1, 257, 257), bc(32, 2, 258, 258, kind="peaked"), bc(16, 3, 259, 259), bc(32, 1, 257, 257, Cq=2, Ck=2),
              bc(32, 3, 257, 130, Cq=4, Ck=1, kind="shifted"), bc(64, 2, 130, 258, kind="flat"), bc(16, 1, 258, 257, table=False),
              bc(64, 1, 257, 257, saved=True, ld_extra=32), bc(64, 2, 258, 258, saved=True, kind="peaked"),
              bc(32, 1, 258, 257, saved=True, wide=True), bc(64, 3, 257, 130, saved=True, layout="head2"),
              bc(16, 2, 130, 257, saved=True, table=False)]
    # the split pair's grid: one 512-thread workgroup per (batch, head, block), 8 ceil(pairs / 8) blocks of them (xcd_grid); a
    # workgroup holds ~160 KB of LDS, so a CU runs one: more items than CUs run in rounds ("one": cus + 1 pairs, pairs % 8 != 0,
    # some workgroups leave at once), fewer in one ("snake": cus // 2 pairs of one block each)
    cases += [bc(16, 1, 129, 129, 1, B=0, H=0, persistent="one"), bc(32, 2, 97, 97, 2, B=0, H=0, persistent="snake", saved=True)]
    # a scale that is not 1 / sqrt(head_dim)
    cases.append(bc(32, 1, 129, 97, 1, Cq=2, Ck=1, scale_mul=0.7, kind="peaked"))
    return cases


ATTENTION_BWD_CASES = _attention_bwd_table()
ATTENTION_BWD_ENTRY_CASES = [c for c in ATTENTION_BWD_CASES if not c.persistent and c.saved and not c.wide and not c.ld_extra and not c.knobs
                             and c.scale_mul == 1.0 and c.table and (c.layout == "contig" or (c.layout == "fused" and c.Sq == c.Sk))]
ATTENTION_BWD_ENTRY_CASES = ([c for c in ATTENTION_BWD_ENTRY_CASES if c.layout == "contig"][:2]
                             + [c for c in ATTENTION_BWD_ENTRY_CASES if c.layout == "fused"][:2])


def _attention_bwd_features(c, cus):
    fam, r = attention_bwd_family(c), attention_bwd_case_route(c, cus)
    rc = attention_bwd_case_resolve(c, cus)
    f = {f"inst {fam} hd{c.hd} p{c.prec}", f"{fam}: Sq {c.Sq}", f"{fam}: Sk {c.Sk}", f"{fam}: mask {c.mask}", f"{fam}: layout {c.layout}",
         f"{fam}: kind {c.kind}", f"{fam}: table {int(c.table)}"}
    if c.dense:
        f.add(f"{fam}: dense mask")
    if not r.unit:
        f.add(f"{fam}: channels {c.Cq}.{c.Ck}")
    if c.ek_extra and c.table:
        f.add(f"{fam}: Ek above the key events")
    if c.wide:
        f.add(f"{fam}: out in a wider buffer")
    if c.saved:
        f.add(f"saved: logits_ld +{c.ld_extra}")
    if c.scale_mul != 1.0:
        f.add("scale is not 1 / sqrt(head_dim)")
    # the products over G
    Rp_ok = r.Rp >= 128
    if c.table and c.prec and r.unit and Rp_ok and c.Sq * rc.B >= 256:
        if c.hd == 64 and c.layout != "batch_first":
            how = ("ISI_NO_GEMM_KERNEL" if c.knobs & ATTN_KNOB_NO_GEMM else "ISI_ATTN_FULL_ZERO" if c.knobs & ATTN_KNOB_FULL_ZERO else
                   "ISI_ATTN_G_FROM_KV=0" if c.knobs & ATTN_KNOB_NO_G_FROM_KV else "g_from_kv" if c.saved else "margins only")
            assert r.gemm_path == (how != "ISI_NO_GEMM_KERNEL") and r.band_only == (how not in ("ISI_NO_GEMM_KERNEL", "ISI_ATTN_FULL_ZERO"))
            assert r.g_from_kv == (how == "g_from_kv")
            if how != "ISI_ATTN_G_FROM_KV=0" or c.saved:
                f.add(f"gemm mask {c.mask}: {how}")
            if c.Sq > 2 * ATTN_G_MARGIN + 1:
                f.add(f"device evidence: {'margins only' if r.band_only else 'full zero'}")
        elif c.hd == 64:
            assert not r.gemm_path
            f.add("no gemm: q_ss != B q_sb")
        else:
            assert not r.gemm_path
            f.add(f"no gemm: head_dim {c.hd}")
            if c.Sq > 2 * ATTN_G_MARGIN + 1:
                f.add("device evidence: full zero where the GEMM declines")
    if c.table and c.prec and r.unit and Rp_ok and c.hd == 64 and c.Sq * rc.B < 256:
        assert not r.gemm_path
        f.add("no gemm: Sq B < 256")
    # tails
    if c.prec and c.mask == 0 and not c.dense:
        if r.tail_q:
            f.add(f"tail query Sq {c.Sq}")
        if r.tail_k:
            f.add(f"tail key Sk {c.Sk}")
        if c.Sq == 259 and c.Sk == 259:
            assert not (r.tail_q or r.tail_k)
            f.add("no tail at 259")
        if c.Sq in ATTN_BWD_TAIL_SIZES and c.table and c.Ck == 2 and not r.tail_q and r.tail_k:
            f.add("tail query declined by Ck = 2")
        if r.tail_q and not r.unit:
            f.add("tail query, several channels per query event")
        if r.tail_q and not r.tail_k:
            f.add("tail query without tail key")
        if r.tail_k and not r.tail_q and c.Ck == 1:
            f.add("tail key without tail query")
        if (r.tail_q or r.tail_k) and not c.table:
            f.add("tail without a table")
        if r.tail_k and r.g_from_kv:
            f.add("tail key with g_from_kv")
        if r.tail_q and r.band_only:
            f.add("tail query into a band-only G")
        if (r.tail_q or r.tail_k) and c.saved and not r.g_from_kv:
            f.add("tail with kept logits, without g_from_kv")
    if c.persistent:
        items = rc.B * rc.H * -(-c.Sq // ATTN_QB)
        f.add("split grid: more items than CUs" if items > cus else "split grid: fewer items than CUs")
        if rc.B * rc.H % 8:
            f.add("split grid: pairs % 8 != 0")
    return f


def attention_bwd_requirements():
    req = [f"inst exact hd{hd} p0" for hd in (16, 32, 64)]
    req += [f"inst {fam} hd{hd} p{p}" for fam in ("split", "saved") for hd in (16, 32, 64) for p in (1, 2, 3)]
    for fam in ATTN_BWD_FAMILIES:
        req += [f"{fam}: Sq {s}" for s in ATTN_SQ] + [f"{fam}: Sk {s}" for s in ATTN_SK] + [f"{fam}: mask {m}" for m in (0, 1, 2)]
        req += [f"{fam}: dense mask", f"{fam}: table 0", f"{fam}: table 1", f"{fam}: Ek above the key events", f"{fam}: out in a wider buffer"]
        req += [f"{fam}: channels {a}.{b}" for a, b in ATTN_CHANNELS] + [f"{fam}: layout {l}" for l in ATTN_LAYOUTS]
        req += [f"{fam}: kind {k}" for k in ATTN_BWD_KINDS]
    req += ["saved: logits_ld +0", "saved: logits_ld +32", "scale is not 1 / sqrt(head_dim)"]
    req += [f"gemm mask {m}: {how}" for m in (0, 1, 2)
            for how in ("margins only", "ISI_ATTN_FULL_ZERO", "ISI_NO_GEMM_KERNEL", "g_from_kv", "ISI_ATTN_G_FROM_KV=0")]
    req += ["device evidence: margins only", "device evidence: full zero", "device evidence: full zero where the GEMM declines"]
    req += ["no gemm: head_dim 32", "no gemm: head_dim 16", "no gemm: Sq B < 256", "no gemm: q_ss != B q_sb"]
    req += [f"tail query Sq {s}" for s in ATTN_BWD_TAIL_SIZES] + [f"tail key Sk {s}" for s in ATTN_BWD_TAIL_SIZES]
    req += ["no tail at 259", "tail query declined by Ck = 2", "tail query, several channels per query event", "tail query without tail key",
            "tail key without tail query", "tail without a table", "tail key with g_from_kv", "tail query into a band-only G",
            "tail with kept logits, without g_from_kv"]
    req += ["split grid: more items than CUs", "split grid: fewer items than CUs", "split grid: pairs % 8 != 0"]
    return req


def attention_bwd_coverage_gaps(cases, cus=ATTN_DEFAULT_CUS):
    """The requirements of the backward's case table (every instantiation; per family the ragged lengths, masks, channel and
    buffer layouts, data kinds; every route of the products over G with the switches; the tails; the grid) no case covers."""
    have = set()
    for c in cases:
        have |= _attention_bwd_features(c, cus)
    return [r for r in attention_bwd_requirements() if r not in have]


AttnBwdData = collections.namedtuple("AttnBwdData", "q k v rel dense scale Ek rel_rows empty_rows dout out lse logits ld forced_row")


def attention_bwd_case_data(c, forced=True):
    """The inputs of a (resolved) case: q, k, v, the table and the dense mask of attention_fwd_case_data (kinds plain, flat,
    shifted; peaked is q x 3 here, and x 1 for a query the mask mode leaves fewer than 8 keys: the forward's q x 6 saturates
    the softmax, as does any factor on a row of two keys, and the gradient of a saturated row vanishes through cancellation --
    its row error, of order 1 for the float32 evaluation too, would be the whole tensor's); dO = randn; out, lse and the kept logits from attention_fwd_spec in FLOAT64, rounded to float32 -- the
    backward is handed tensors no kernel of the project made.  logits [B,H,Sq,ld] hold NaN at every pair the mask mode
    leaves out and in the columns from Sk on ("entries of masked pairs are never read"), -inf where the dense mask is.
    forced: one more row (Sq // 3, for Sq >= 33) is made empty by lse = ATTN_EMPTY_LSE alone, and the given `out` of a row
    with a single live key (the first causal row, every row of a one-key call) is HALF the forward's: with the forward's own
    out such a row has P = 1 and dO v = D identically, so dS = 0 and its dq would hold rounding noise of size 1e-8 against a
    float64 reference of size 1e-17 -- a row that measures nothing and, as the largest row error of the tensor, hides every
    other row.  The operation is a function of the given tensors; with out / 2 that row's dS = P (dO v) scale / 2 is as well
    conditioned as any other and shows that the given out is what is read."""
    import zlib
    fc = _attention_bwd_fwd_case(c)
    d = attention_fwd_case_data(fc._replace(kind="plain") if c.kind == "peaked" else fc)
    if c.kind == "peaked":
        few = attention_allowed(c.Sq, c.Sk, c.mask).sum(-1) < 8
        d = d._replace(q=d.q * torch.where(few, 1.0, 3.0)[:, None, None, None])
    scale = float(np.float32(d.scale * c.scale_mul))
    fwd = attention_fwd_spec(d.q, d.k, d.v, d.rel, c.H, c.Cq, c.Ck, d.Ek, c.mask, d.dense, scale)
    gen = torch.Generator().manual_seed(zlib.crc32(("dO " + attention_bwd_case_id(c._replace(B=0, H=0) if c.persistent else c)).encode()))
    dout = torch.randn(c.Sq, c.B, c.H, c.hd, generator=gen)
    out = fwd.out.float().clone()
    lse = fwd.lse.float().clone()
    empty, forced_row = set(d.empty_rows), None
    if forced:
        out[(fwd.allowed & (fwd.logits2 > float("-inf"))).sum(-1) == 1] *= 0.5
        if c.Sq >= 33:
            forced_row = c.Sq // 3
            lse[:, :, forced_row] = ATTN_EMPTY_LSE
            empty.add(forced_row)
    out = out.permute(2, 0, 1, 3).contiguous()
    ld = (c.Sk + 31) // 32 * 32 + c.ld_extra
    logits = torch.full((c.B, c.H, c.Sq, ld), float("nan"))
    logits[..., :c.Sk] = torch.where(fwd.allowed, fwd.logits2.float(), torch.full((), float("nan")))
    return AttnBwdData(d.q, d.k, d.v, d.rel, d.dense, scale, d.Ek, d.rel_rows, sorted(empty), dout, out, lse, logits, ld, forced_row)


AttnBwdRefs = collections.namedtuple("AttnBwdRefs", "spec f32 model yard route")


def attention_bwd_args(c, d, saved):
    return (d.q, d.k, d.v, d.rel, c.H, c.Cq, c.Ck, d.Ek, c.mask, d.dense, d.scale, d.dout, d.out, d.lse, d.logits if saved else None)


def attention_bwd_refs(c, d, route, models=True):
    """spec, float32 evaluation, the split pair's model (None on the exact route) and the yardstick of the hold: the float32
    evaluation on the exact route; on the split routes per element the worse of it and the model -- but the float32
    evaluation ALONE on what the exact-fp32 one-row kernels produce by themselves: dk and dv of the last route.tail_k keys,
    and dq of the last route.tail_q queries where there is no table (with one, the row also receives G E from the three-term
    product like every other row: the model says so and the larger of the two applies)."""
    a = attention_bwd_args(c, d, route.saved)
    spec = attention_bwd_spec(*a)
    f32 = AttnBwd(*(None if t is None else t.double() for t in attention_bwd_f32(*a)))
    assert all(t is None or bool(torch.isfinite(t).all()) for t in f32), "the float32 yardstick is not finite on this data"
    model, yard = None, f32
    if route.split and models:
        model = attention_bwd_model(*a, c.prec, route.saved, tail_q=route.tail_q, tail_k=route.tail_k, g_from_kv=route.g_from_kv)
        yard = AttnBwd(*(None if s is None else larger_error(f, m, s) for f, m, s in zip(f32, model, spec)))
        if route.tail_k:
            yard.dk[:, :, -route.tail_k:], yard.dv[:, :, -route.tail_k:] = f32.dk[:, :, -route.tail_k:], f32.dv[:, :, -route.tail_k:]
        if route.tail_q and not route.has_e:
            yard.dq[:, :, -route.tail_q:] = f32.dq[:, :, -route.tail_q:]
    return AttnBwdRefs(spec, f32, model, yard, route)


@functools.lru_cache(maxsize=2)
def attention_bwd_case_refs(c, cus=ATTN_DEFAULT_CUS):
    """(resolved case, data, refs) of a case on a device of `cus` CUs; computed once per case."""
    r = attention_bwd_case_resolve(c, cus)
    d = attention_bwd_case_data(r)
    return r, d, attention_bwd_refs(r, d, attention_bwd_case_route(c, cus))


def attention_bwd_hold(got, refs, what, yard=None, margin=ROW_OPS_MARGIN):
    """The hold of the attention backward: per output (dq, dk, dv, d_rel; rows = the hd values of one query / key / table
    row) every element finite, a row the spec finds exactly 0 (an empty query row, a key no live query reaches, a table
    row no allowed pair selects) exactly 0, and compare_rows with the project's margin and floor.  The rows of the one-row
    kernels (the last route.tail_q queries of dq, the last route.tail_k keys of dk and dv) are blocks of their own.
    Returns {"dq" | "tail dq" | ...: RowCheck}; raises AssertionError at the first failure."""
    spec, yard, r = refs.spec, yard or refs.yard, refs.route
    checks = {}
    for name, tail in (("dq", r.tail_q), ("dk", r.tail_k), ("dv", r.tail_k), ("d_rel", 0)):
        s, y, g = getattr(spec, name), getattr(yard, name), getattr(got, name)
        if s is None:
            assert g is None, f"{what}: {name} without a table"
            continue
        assert g is not None, f"{what}: no {name}"
        g = torch.as_tensor(g).detach().cpu()
        assert g.shape == s.shape, f"{what}: {name} {tuple(g.shape)} against {tuple(s.shape)}"
        assert bool(torch.isfinite(g).all()), f"{what}: {name} is not finite"
        zero = (s == 0).all(-1)
        assert bool((g[zero] == 0).all()), f"{what}: a row of {name} the spec finds exactly 0 is not 0"
        n = s.shape[-2]
        for block, rows in (("", slice(0, n - tail)), ("tail ", slice(n - tail, n))):
            if rows.start != rows.stop:
                checks[block + name] = compare_rows(g[..., rows, :], s[..., rows, :], y[..., rows, :], f"{what} {block}{name}", margin)
    return checks


# ---------------------------------------------------------------------------------------------------------------------
# Float64 specification, float32 yardstick, split-product models, route mirror and case table of the implicit-GEMM
# convolutions (csrc/conv_igemm_f32.hip through isi_conv2d_f32 / isi_conv2d_gated_f32 / isi_conv_transpose2d_k4s2_f32 and
# its gated form), in the style of the blocks above: plain torch on the CPU, no autograd and none of the project's kernels.
# A convolution is an im2col product followed by an epilogue,
#     v = rows W2d^T + bias + residual;  ReLU;  gate > 0 ? v : 0                                  (the epilogue's order)
# rows [M, K] with M = B OH OW pixels (image-major) and K = KH KW Cin in the packed weight's order k = (kh KW + kw) Cin + c
# (taps outer, channels inner; channels = cat(x, x2)), W2d [Cout, K].  ConvTranspose2d(4, 2, 1) is four such products, one
# per output phase (py, px) = (oy % 2, ox % 2) with M = B H W: tap (ty, tx) of a phase reads the input at
# (my - (1 - py) + ty, mx - (1 - px) + tx) and is torch's tap (3 - py - 2 ty, 3 - px - 2 tx) (csrc/pack.hip).
# Tensors are logical [B, C, H, W] whatever their storage.  A "row" for compare_rows is one output channel: `conv_rows`.
# tests/test_conv_igemm_host.py holds the spec to torch's float64 convolutions and their autograd and shows what the
# comparison rejects; tests/test_conv_igemm_gpu.py holds the kernels to it on every route.
CONV_FLAGS = {"relu": 1, "bf16x3": 2, "bf16x6": 4, "f16x3": 8, "w16": 16, "in0_pair": 32, "in1_pair": 64, "out_pair": 128,
              "gate_pair": 512}                                      # ISI_CONV_* of include/isi_hip.h
CONV_PREC_FLAGS = {0: 0, 1: 2, 2: 4, 3: 8, 4: 24}                    # vqvae/_ops.py _prec_flag: the `bf16x3` argument -> flag bits
CONV_E_INVALID, CONV_E_UNSUPPORTED = -1, -4
CONV_FAMILIES = {1: "igemm", 2: "pair-dma", 3: "conv-first", 4: "gemm", 5: "convT-small", 6: "convT-small-pair", 7: "convT-pair"}
CONV_LOADERS = ("uniform", "dual", "gather")
CONV_BM = 128                                                        # rows of every tile of conv_igemm_f32_kernel
ConvRoute = collections.namedtuple("ConvRoute", "family bn loader prec outp slice_major")


def conv_route_pack(r):
    """The int of isi_conv2d_route / isi_conv_transpose2d_k4s2_route (include/isi_hip.h)."""
    return r.family | (r.bn // 32) << 4 | r.loader << 8 | r.prec << 10 | r.outp << 13 | r.slice_major << 14


def conv_route_unpack(v):
    assert v > 0, f"status {v}, not a route"
    return ConvRoute(v & 15, (v >> 4 & 15) * 32, v >> 8 & 3, v >> 10 & 7, v >> 13 & 1, v >> 14 & 1)


def conv_route_name(v):
    if v <= 0:
        return f"refused {v}"
    r = conv_route_unpack(v)
    if r.family != 1:
        return CONV_FAMILIES[r.family]
    return (f"igemm 128x{r.bn} {CONV_LOADERS[r.loader]} prec {r.prec}{' pair-out' if r.outp else ''}"
            f"{' slice-major' if r.slice_major else ''}")


# A case.  op "conv" | "convT" (k 4, stride 2, pad 1, one source); B, H, W: the layer INPUT; mode: the precision asked for
# (the `bf16x3` argument of vqvae/_ops.py: 0 exact fp32, 1 bf16x3, 2 bf16x6, 3 f16x3, 4 f16x3 with pack-time weight pieces);
# src0 / src1 / out / res: storage of that tensor (`conv_layout`): "nhwc" dense channels-last, "nchw" dense NCHW, "off1"
# channels-last one float off a 16-byte boundary, "row" channels-last with two floats between rows (row stride % 4 != 0),
# "slice" a channel slice [4, 4 + C) of a channels-last tensor of C + 8 channels; gate None | "f32" | "pair" (laid out like
# the output); pairs: which of source 0 ("0"), source 1 ("1") and the output ("o") are in the pair format; knobs: execution
# switches ((name, value), ...) set around the launch.
ConvCase = collections.namedtuple("ConvCase", "op c0 c1 cout k stride pad B H W mode src0 src1 out res gate bias relu pairs knobs")
ConvLayout = collections.namedtuple("ConvLayout", "shape strides offset storage")     # logical [B, C, H, W]; floats


def _cv(c0, cout, k, stride, pad, B, H, W, mode=0, c1=0, src0="nhwc", src1="nhwc", out="nhwc", res=None, gate=None, bias=True,
        relu=False, pairs="", knobs=()):
    return ConvCase("conv", c0, c1, cout, k, stride, pad, B, H, W, mode, src0, src1 if c1 else None, out, res, gate, bias, relu, pairs,
                    tuple(knobs))


def _ct(cin, cout, B, H, W, mode=0, src0="nhwc", out="nhwc", gate=None, bias=True, relu=False, pairs="", knobs=()):
    return ConvCase("convT", cin, 0, cout, 4, 2, 1, B, H, W, mode, src0, None, out, None, gate, bias, relu, pairs, tuple(knobs))


def conv_out_hw(c):
    if c.op == "convT":
        return 2 * c.H, 2 * c.W
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def conv_case_id(c):
    src = f"{c.c0}+{c.c1}" if c.c1 else f"{c.c0}"
    lay = c.src0 + (f"+{c.src1}" if c.c1 else "")
    extra = "".join([f"-res_{c.res}" if c.res else "", f"-gate_{c.gate}" if c.gate else "", "" if c.bias else "-nobias",
                     "-relu" if c.relu else "", f"-pairs_{c.pairs}" if c.pairs else "",
                     "".join(f"-{n}={v}" for n, v in c.knobs)])
    return f"{c.op}{src}to{c.cout}k{c.k}s{c.stride}p{c.pad}-{c.B}x{c.H}x{c.W}-m{c.mode}-{lay}-to_{c.out}{extra}"


def _conv_tensor_layout(kind, B, Cc, H, W):
    if kind == "nhwc":
        return ConvLayout((B, Cc, H, W), (H * W * Cc, 1, W * Cc, Cc), 0, B * H * W * Cc)
    if kind == "nchw":
        return ConvLayout((B, Cc, H, W), (Cc * H * W, H * W, W, 1), 0, B * Cc * H * W)
    if kind == "off1":
        return ConvLayout((B, Cc, H, W), (H * W * Cc, 1, W * Cc, Cc), 1, B * H * W * Cc + 4)
    if kind == "row":
        sh = W * Cc + 2
        return ConvLayout((B, Cc, H, W), (H * sh, 1, sh, Cc), 0, B * H * sh)
    assert kind == "slice", kind
    Cw = Cc + 8
    return ConvLayout((B, Cc, H, W), (H * W * Cw, 1, W * Cw, Cw), 4, B * H * W * Cw)


def conv_layout(c):
    """{"src0", "src1", "out", "res", "gate": ConvLayout or None}: where every tensor of the case lies in its storage (a flat
    buffer whose first float is 16-byte aligned).  The gate is laid out exactly like the output, as the C-ABI requires."""
    OH, OW = conv_out_hw(c)
    out = _conv_tensor_layout(c.out, c.B, c.cout, OH, OW)
    return {"src0": _conv_tensor_layout(c.src0, c.B, c.c0, c.H, c.W),
            "src1": _conv_tensor_layout(c.src1, c.B, c.c1, c.H, c.W) if c.c1 else None,
            "out": out, "res": _conv_tensor_layout(c.res, c.B, c.cout, OH, OW) if c.res else None,
            "gate": out if c.gate else None}


def conv_case_flags(c, mode=None, gate="case", pairs=None):
    """The flag word of the case's launch (other precision / gate / pair formats: those of the variant launch)."""
    pairs = c.pairs if pairs is None else pairs
    gate = c.gate if gate == "case" else gate
    f = int(c.relu) | CONV_PREC_FLAGS[c.mode if mode is None else mode]
    f |= (32 if "0" in pairs else 0) | (64 if "1" in pairs else 0) | (128 if "o" in pairs else 0)
    return f | (512 if gate == "pair" else 0)


def _extent(l):
    return sum((n - 1) * s for n, s in zip(l.shape, l.strides)) + 1


def conv_route(c, mode=None, gate="case", pairs=None, knobs=None):
    """Mirror of the decisions of conv2d_batched_f32 / conv_transpose2d_k4s2_f32 and of conv_route (csrc/conv_igemm_f32.hip)
    for a case with a 16-byte aligned packed weight: the int isi_conv2d_route / isi_conv_transpose2d_k4s2_route returns -- the
    packed route, or the negative status of a refusal.  `knobs`: {name: value} of the execution switches in force (default:
    the case's).  The rules it spells out: only the uniform loader runs split products (a split flag on a dual-source or
    gather launch runs exact fp32); split products need K >= 128 (bf16x3: K >= 64 where Cout > 32); there is no
    pack-time-pieces instance at Cout <= 32 (mode 4 runs PREC 3 there)."""
    kn = dict(c.knobs if knobs is None else knobs)
    flags = conv_case_flags(c, mode, gate, pairs)
    has_gate = (c.gate if gate == "case" else gate) is not None
    lay = conv_layout(c)
    s0, s1, dst, res = lay["src0"], lay["src1"], lay["out"], lay["res"]
    split = 2 if flags & 4 else 3 if flags & 8 else 1 if flags & 2 else 0
    in0p, in1p, outp, w16, gate_pair = bool(flags & 32), bool(flags & 64 and c.c1), bool(flags & 128), bool(flags & 16), bool(flags & 512)
    al = lambda l: l.offset % 4 == 0
    big = 1 << 30
    OH, OW = conv_out_hw(c)

    def vec_of(l, Cc):
        return l.strides[1] == 1 and Cc % 4 == 0 and al(l) and l.strides[0] % 4 == 0 and l.strides[2] % 4 == 0 and l.strides[3] % 4 == 0

    def dense_nhwc(l, Cc, h, w):
        return (l.strides[1] == 1 and (w == 1 or l.strides[3] == Cc) and (h == 1 or l.strides[2] == w * Cc)
                and (c.B == 1 or l.strides[0] == h * w * Cc))

    if c.op == "convT":
        Cin, small = c.c0, 1 <= c.cout <= 4 and c.c0 in (32, 64)
        if has_gate and (small or flags & (32 | 128)):
            return CONV_E_UNSUPPORTED
        if _extent(s0) >= big or _extent(dst) >= big:
            return CONV_E_UNSUPPORTED
        d_in = dense_nhwc(s0, Cin, c.H, c.W)
        if small:
            if flags & 32:
                ok = not outp and w16 and split == 3 and d_in and Cin == 64 and c.cout <= 2 and al(s0)
                return 6 if ok else CONV_E_UNSUPPORTED
            return CONV_E_UNSUPPORTED if outp else 5
        d_out = (dst.strides[1] == 1 and dst.strides[3] == c.cout and dst.strides[2] == 2 * c.W * c.cout
                 and (c.B == 1 or dst.strides[0] == 4 * c.H * c.W * c.cout))
        pair_ok = not kn.get("ISI_NO_CONVT_PAIR_KERNEL") and Cin >= 16 and Cin % 16 == 0 and c.cout % 64 == 0 and c.cout <= 1024
        if flags & 32 and w16 and split == 3 and d_in and d_out and pair_ok and al(s0) and al(dst):
            return 7
        K, KH, KW, nphase, convT, two, C0, uniform = 4 * Cin, 2, 2, 4, True, False, Cin, True
        scalar, M, in1p, has_res = not vec_of(s0, Cin), c.B * c.H * c.W, False, False
    else:
        if has_gate and flags & (32 | 64 | 128):
            return CONV_E_UNSUPPORTED
        if OH <= 0 or OW <= 0:
            return CONV_E_INVALID
        two = c.c1 > 0
        if two and s1.strides[1] != 1:
            return CONV_E_UNSUPPORTED
        if max(_extent(s0), _extent(s1) if two else 1, _extent(dst), _extent(res) if res else 1) >= big:
            return CONV_E_UNSUPPORTED
        d_out = (dst.strides[1] == 1 and dst.strides[3] == c.cout and dst.strides[2] == OW * c.cout
                 and dst.strides[0] == OH * OW * c.cout and al(dst))
        if ((not has_gate or (not flags & (128 | 512))) and not kn.get("ISI_NO_CONV_FIRST") and not two and not res
                and (c.c0, c.k, c.stride, c.pad) == (2, 4, 2, 1) and c.cout in (32, 64) and d_out):
            return CONV_E_UNSUPPORTED if flags & (32 | 64) else 3
        if (not (has_gate and gate_pair) and not two and (c.k, c.stride, c.pad, c.B, c.H) == (1, 1, 0, 1, 1) and s0.strides[1] == 1
                and dst.strides[1] == 1 and (not res or res.strides[1] == 1) and not flags & (32 | 64 | 128)
                and split in (1, 3) and c.c0 % 32 == 0 and c.c0 >= 128 and c.cout > 32 and c.W >= 256
                and al(s0) and s0.strides[3] % 4 == 0 and not kn.get("ISI_NO_GEMM_KERNEL")):
            return 4
        if res and (in0p or in1p or outp):
            return CONV_E_UNSUPPORTED
        K, KH, KW, nphase, convT, C0 = c.k * c.k * (c.c0 + c.c1), c.k, c.k, 1, False, c.c0
        uniform = not two or (c.c0 % 32 == 0 and c.c1 % 32 == 0)
        scalar = not (vec_of(s0, c.c0) and c.c1 % 4 == 0 and (not two or vec_of(s1, c.c1)))
        M, has_res = c.B * OH * OW, bool(res)
    # ---- conv_route of csrc/conv_igemm_f32.hip
    Cin, cout = c.c0 + c.c1, c.cout
    loader = 2 if scalar else 0 if uniform else 1
    slice_major = int(loader == 0 and KH * KW > 1 and C0 % 32 == 0 and Cin % 32 == 0)
    dma_shape = bool(kn.get("ISI_CONV_PAIR_ALL")) or (not convT and K >= 256)
    dma_kernel = (not kn.get("ISI_NO_CONV_PAIR_KERNEL") and C0 > 0 and C0 % 32 == 0 and (Cin - C0) % 32 == 0 and cout % 64 == 0
                  and 1 <= KH * KW <= 16)
    if (dma_shape and split == 3 and w16 and loader == 0 and in0p and (not two or in1p) and not has_res and dst.strides[1] == 1
            and dma_kernel and KH <= 4 and KW <= 4 and M < 1 << 24):
        return 2
    if (in0p or in1p or outp) and not (split == 3 and w16 and loader == 0 and cout > 32 and K >= 128):
        return CONV_E_UNSUPPORTED
    if split and loader == 0 and cout <= 32 and K >= 128 and not (outp or in0p or in1p):
        return conv_route_pack(ConvRoute(1, 32, 0, split, 0, slice_major))
    if split and loader == 0 and cout > 32 and (K >= 128 or (split == 1 and K >= 64 and not (in0p or in1p or outp))):
        tiles128 = -(-M // 128) * -(-cout // 128) * nphase
        bn = 64 if cout <= 64 or tiles128 < 640 else 128
        prec = 4 if split == 3 and w16 else split
        if prec == 4 and outp and (dst.strides[1] != 1 or cout % 8):
            return CONV_E_UNSUPPORTED
        return conv_route_pack(ConvRoute(1, bn, 0, prec, int(prec == 4 and outp), slice_major))
    return conv_route_pack(ConvRoute(1, 32 if cout <= 32 else 64 if cout <= 64 else 128, loader, 0, 0, slice_major))


# ---- the specification
def _conv_cat(x, x2, dtype, pair0=False, pair1=False, swap_sources=False):
    """cat(x, x2) [B, Cin, H, W] in `dtype`; a pair-format source holds pair_decode_host(pair_encode_host(x)) (groups of 8
    channels of channels-last storage)."""
    def one(t, pair):
        t = torch.as_tensor(t).detach().cpu()
        if pair:
            t = pair_decode_host(pair_encode_host(t.float().permute(0, 2, 3, 1).contiguous())).permute(0, 3, 1, 2)
        return t.to(dtype)
    x = one(x, pair0)
    if x2 is None:
        return x
    x2 = one(x2, pair1)
    return torch.cat([x2, x] if swap_sources else [x, x2], dim=1)


def _conv_gemms(xc, w, k, stride, pad, transposed, pad_shift=False):
    """The products of a convolution: [(rows [B, L, K], W2d [Cout, K], phase (py, px) or None)] in the dtype of xc, K in the
    packed order.  `pad_shift` is a host-test mutant: the left padding one more, the right one less."""
    B, Cin = xc.shape[:2]
    w = torch.as_tensor(w).detach().cpu().to(xc.dtype)

    def rows_of(src, kk, **kw):
        cols = torch.nn.functional.unfold(src, kk, **kw)                             # [B, Cin kk kk, L], channel-major
        return cols.reshape(B, Cin, kk * kk, -1).permute(0, 3, 2, 1).reshape(B, cols.shape[-1], kk * kk * Cin)
    if not transposed:
        if pad_shift:
            assert pad >= 1
            rows = rows_of(torch.nn.functional.pad(xc, (pad + 1, pad - 1, pad, pad)), k, stride=stride)
        else:
            rows = rows_of(xc, k, padding=pad, stride=stride)
        return [(rows, w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), None)]
    assert (k, stride, pad) == (4, 2, 1)
    out = []
    for py in range(2):
        for px in range(2):
            xp = torch.nn.functional.pad(xc, (1 - px, px, 1 - py, py))
            wp = w[:, :, [3 - py, 1 - py]][:, :, :, [3 - px, 1 - px]]                # [Cin, Cout, ty, tx]
            out.append((rows_of(xp, 2), wp.permute(1, 2, 3, 0).reshape(w.shape[1], -1), (py, px)))
    return out


def _conv_eval(op_dtype, acc_dtype, x, x2, w, bias, k, stride, pad, transposed=False, res=None, relu=False, gate=None,
               gate_pair=False, pair0=False, pair1=False, prod=None, drop_last_chunk=False, pad_shift=False, border_tap=False,
               swap_sources=False, seam_tile=0, bias_tile=0, res_after_relu=False, gate_ge=False, gate_wrong_half=False,
               swap_phases=False):
    """[B, Cout, OH, OW] in acc_dtype: operands built in op_dtype, every product by `prod(rows2d, W2d)` (default: the matmul
    in op_dtype), the epilogue in acc_dtype.  The switches from `drop_last_chunk` on are the host tests' mutants."""
    xc = _conv_cat(x, x2, op_dtype, pair0, pair1, swap_sources)
    B, _, H, W = xc.shape
    OH, OW = (2 * H, 2 * W) if transposed else ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)
    out = None
    for rows, W2d, phase in _conv_gemms(xc, w, k, stride, pad, transposed, pad_shift):
        L, K = rows.shape[1:]
        if border_tap:                                   # the pixels of the last output column lose their tap (0, kw) on column W - 1
            assert not transposed
            kw = W - 1 - ((OW - 1) * stride - pad)
            assert 0 <= kw < k
            rows = rows.clone()
            Cin = K // (k * k)
            rows[:, OW - 1::OW, kw * Cin:(kw + 1) * Cin] = 0
        r2 = rows.reshape(B * L, K)
        if seam_tile:                                    # every row of a tile reads the image of the tile's first row
            m = torch.arange(B * L)
            r2 = r2[(m // seam_tile * seam_tile) // L * L + m % L]
        if drop_last_chunk:
            r2, W2d = r2[:, :K // 32 * 32], W2d[:, :K // 32 * 32]
        p = (r2 @ W2d.t() if prod is None else prod(r2, W2d)).to(acc_dtype)
        if phase is None:
            out = p.reshape(B, OH, OW, -1)
        else:
            if out is None:
                out = torch.zeros(B, OH, OW, p.shape[-1], dtype=acc_dtype)
            py, px = (phase[1], phase[0]) if swap_phases else phase
            out[:, py::2, px::2] = p.reshape(B, H, W, -1)
    cout = out.shape[-1]
    nhwc = lambda t: torch.as_tensor(t).detach().cpu().to(acc_dtype).permute(0, 2, 3, 1)
    if bias is not None:
        b = torch.as_tensor(bias).detach().cpu().to(acc_dtype).clone()
        if bias_tile:
            b[(cout - 1) // bias_tile * bias_tile:] = 0
        out = out + b
    if res is not None and not res_after_relu:
        out = out + nhwc(res)
    if relu:
        out = torch.where(out < 0, torch.zeros_like(out), out)          # (NaN stays NaN, as the kernel keeps it)
    if res is not None and res_after_relu:
        out = out + nhwc(res)
    if gate is not None:
        out = torch.where(conv_gate_mask(gate, gate_pair, gate_ge, gate_wrong_half).permute(0, 2, 3, 1), out, torch.zeros_like(out))
    return out.permute(0, 3, 1, 2)


def conv_gate_mask(gate, gate_pair=False, gate_ge=False, gate_wrong_half=False):
    """[B, Cout, OH, OW] bool: where the gated epilogue lets a value through.  fp32 gate: gate > 0.  Pair-format gate: the
    activation its pairs decode to, > 0 -- a value so small that its hi piece f16(4 x) rounds to zero decodes to zero and is
    closed.  Mutants: `gate_ge` (>=), `gate_wrong_half` (an odd channel reads the half-word of the even channel below it)."""
    g = torch.as_tensor(gate).detach().cpu().float()
    if gate_pair:
        g = pair_decode_host(pair_encode_host(g.permute(0, 2, 3, 1).contiguous())).permute(0, 3, 1, 2)
    m = g >= 0 if gate_ge else g > 0
    if gate_wrong_half:
        m = m.clone()
        m[:, 1::2] = m[:, 0::2][:, :m[:, 1::2].shape[1]]
    return m


def conv_spec(x, x2, w, bias, k, stride, pad, transposed=False, res=None, relu=False, gate=None, gate_pair=False, pair0=False,
              pair1=False):
    """Float64 closed form of isi_conv2d_f32 on cat(x, x2) (w [Cout, Cin, k, k]) and, `transposed`, of
    isi_conv_transpose2d_k4s2_f32 (w [Cin, Cout, 4, 4]): bias, the residual added before the ReLU, the ReLU, the gate last.
    A pair-format output holds the pair encoding of the float32 result: the spec is the same value (the comparison decodes)."""
    return _conv_eval(torch.float64, torch.float64, x, x2, w, bias, k, stride, pad, transposed, res, relu, gate, gate_pair, pair0, pair1)


def conv_f32(x, x2, w, bias, k, stride, pad, transposed=False, res=None, relu=False, gate=None, gate_pair=False, pair0=False,
             pair1=False, out_pair=False, **mutants):
    """The same in float32 torch: the yardstick of the exact-fp32 instances, half of the split instances', and what the host
    tests apply their mutants to.  `out_pair`: rounded to what the pair format holds of it."""
    v = _conv_eval(torch.float32, torch.float32, x, x2, w, bias, k, stride, pad, transposed, res, relu, gate, gate_pair, pair0, pair1,
                   **mutants)
    return pair_round_f16(v) if out_pair else v


def conv_six_term_product(rows, W2d, drop_mid=False):
    """Float64 value of the six terms PREC 2 keeps (conv_igemm_f32_kernel: "lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi"
    of the three-piece bf16 split of both operands).  `drop_mid`: the three terms without a mid piece -- not the terms of any
    mode (the three-term mode splits in TWO pieces), a host-test mutant."""
    (ah, am, al), (bh, bm, bl) = bf16_pieces(rows, 3), bf16_pieces(W2d, 3)
    s = ah @ bh.t() + ah @ bl.t() + al @ bh.t()
    return s if drop_mid else s + ah @ bm.t() + am @ bh.t() + am @ bm.t()


def conv_split_model(x, x2, w, bias, k, stride, pad, transposed=False, res=None, relu=False, gate=None, gate_pair=False,
                     pair0=False, pair1=False, mode=1, drop=None):
    """Float64 evaluation of the terms a split mode keeps of every product, on the float32 im2col rows and weights: modes 1
    and 3 / 4 by `linear_split_model` ("bf16" / "f16": lo.hi + hi.lo + hi.hi), mode 2 by `conv_six_term_product`; the epilogue
    in float64.  Its distance from conv_spec is the truncation the mode accepts by design.  `drop`: linear_split_model's
    mutant switch (a two-term product)."""
    if mode == 2:
        prod = conv_six_term_product
    else:
        prod = lambda r, W2d: linear_split_model(r, W2d, {1: "bf16", 3: "f16", 4: "f16"}[mode], drop)
    return _conv_eval(torch.float32, torch.float64, x, x2, w, bias, k, stride, pad, transposed, res, relu, gate, gate_pair, pair0,
                      pair1, prod=prod)


def conv_yardstick(prec, spec, f32, model=None):
    """The yardstick of an instance's product mode (PREC of the route, not the mode asked for: a downgraded launch is held
    to what it runs), after conv_wgrad_yardstick: 0 the float32 evaluation; 1, 3 and 4 per element the worse of the float32
    evaluation and the three-term model; 2 the six-term model."""
    if prec == 0:
        return f32
    if prec == 2:
        return model
    assert prec in (1, 3, 4), prec
    return larger_error(f32, model, spec)


def conv_rows(t):
    """[B, Cout, OH, OW] -> [Cout, B OH OW]: a row for compare_rows is one output channel."""
    t = torch.as_tensor(t).detach().cpu()
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


CONV_GATE_TINY = (2.0 ** -26, 2.0 ** -27, 2.0 ** -30, 1e-12)     # 4 x 2^-26 = the smallest f16: open; the others' hi piece is 0


def conv_case_data(c):
    """{"x", "x2", "w", "bias", "res", "gate"} float32 on the CPU, logical [B, C, H, W], seeded from the case's shape: source 0
    randn (an output gradient), source 1 rectified randn (an activation), w = randn / sqrt(K), and a gate of rectified randn
    -- about half zeros -- with -0.0, negatives and CONV_GATE_TINY sprinkled over it, all four at the head and the tail."""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(repr(c[:10]).encode()))
    OH, OW = conv_out_hw(c)
    Cin = c.c0 + c.c1
    d = {"x": torch.randn(c.B, c.c0, c.H, c.W, generator=g),
         "x2": torch.relu(torch.randn(c.B, c.c1, c.H, c.W, generator=g)) if c.c1 else None}
    wshape = (c.c0, c.cout, 4, 4) if c.op == "convT" else (c.cout, Cin, c.k, c.k)
    d["w"] = torch.randn(*wshape, generator=g) / math.sqrt((4 if c.op == "convT" else c.k * c.k) * Cin)
    d["bias"] = torch.randn(c.cout, generator=g) if c.bias else None
    d["res"] = torch.randn(c.B, c.cout, OH, OW, generator=g) if c.res else None
    d["gate"] = None
    if c.gate:
        y = torch.relu(torch.randn(c.B, OH, OW, c.cout, generator=g)).reshape(-1)
        special = torch.tensor([-0.0, -1.5, *CONV_GATE_TINY, 0.75])
        n = y.numel()
        where = torch.cat([torch.arange(min(n, 7)), torch.arange(7, max(n, 7), 11), torch.arange(max(n - 7, 0), n)])
        y[where] = special[where % 7]
        d["gate"] = y.reshape(c.B, OH, OW, c.cout).permute(0, 3, 1, 2)
    return d


ConvRefs = collections.namedtuple("ConvRefs", "spec f32 models")
_conv_refs_cache = {}


def conv_case_args(c, d, gate="case"):
    """Positional and keyword arguments of conv_spec / conv_f32 / conv_split_model for a case's launch (gate=None: the plain
    launch of a gated case)."""
    gate_kind = c.gate if gate == "case" else gate
    return ((d["x"], d["x2"], d["w"], d["bias"], c.k, c.stride, c.pad),
            dict(transposed=c.op == "convT", res=d["res"], relu=c.relu, gate=d["gate"] if gate_kind else None,
                 gate_pair=gate_kind == "pair", pair0="0" in c.pairs, pair1="1" in c.pairs))


def conv_case_refs(c, modes=None):
    """(spec, float32 evaluation, {mode: model}) of a case, each computed once per process and left unchanged.  `modes`: the
    split modes whose model is wanted (default: the PREC the case's route runs)."""
    key = c._replace(mode=0, knobs=())
    if key not in _conv_refs_cache:
        a, kw = conv_case_args(c, conv_case_data(c))
        _conv_refs_cache[key] = ConvRefs(conv_spec(*a, **kw), conv_f32(*a, out_pair="o" in c.pairs, **kw), {})
    refs = _conv_refs_cache[key]
    if modes is None:
        r = conv_route(c)
        modes = [conv_route_unpack(r).prec] if r > 0 and r & 15 == 1 else []
    for m in modes:
        m = 3 if m == 4 else m                             # (the pack-time pieces are the same pieces)
        if m and m not in refs.models:
            a, kw = conv_case_args(c, conv_case_data(c))
            refs.models[m] = conv_split_model(*a, mode=m, **kw)
    return refs


def conv_refs_yardstick(refs, prec):
    return conv_yardstick(prec, refs.spec, refs.f32, refs.models.get(3 if prec == 4 else prec))


# ---- the case table.  Shapes are the smallest that still reach what the comment names; M = B OH OW.
CONV_BIG_CASES = [
    # the narrow / wide switch at tiles128 = 640: four phases x 160 row tiles (M = 20447, odd map; Cin = 32: K = 128, Cout = 96:
    # ragged weight rows in the 128-wide tile) = 640 -> wide; 1x1 128 -> 264 (three column tiles) x 213 row tiles = 639 -> narrow
    # (the wide instances of modes 2 .. 4 and the wide pair-format output need 640 tiles too: the same data and spec again)
    *[_ct(32, 96, 1, 127, 161, mode=m) for m in (1, 2, 3, 4)], _ct(32, 96, 1, 127, 161, mode=4, pairs="o"),
    _cv(128, 264, 1, 1, 0, 1, 142, 192, mode=1),
    # the epilogues of the wide split instance (two column tiles per wave; production: the 128 -> 128 input gradients at a
    # large batch): 214 row tiles x three column tiles = 642, and the four phases once more with a gate
    _cv(128, 264, 1, 1, 0, 1, 143, 191, mode=1, res="nchw", gate="f32", bias=False),
    _cv(128, 264, 1, 1, 0, 1, 143, 191, mode=1, res="nhwc", gate="pair", relu=True),
    _ct(32, 96, 1, 127, 161, mode=1, gate="pair", bias=False),
]


def _conv_table():
    t = []
    # -- loaders x tile widths, exact fp32 (and the Cout edges 1, 33, 40, 72, 130: unused columns / weight rows of the last tile)
    t += [_cv(4, 1, 3, 1, 1, 1, 5, 7),                                  # uniform 128x32, K = 36: zero-padded tail, tap-major
          _cv(8, 33, 3, 1, 1, 1, 5, 7), _cv(16, 40, 3, 1, 1, 2, 5, 7), _cv(32, 72, 3, 1, 1, 1, 5, 7), _cv(4, 130, 3, 1, 1, 1, 5, 7),
          _cv(48, 16, 3, 1, 1, 1, 5, 7),                                # a chunk straddles taps: C = 48, tap-major
          _cv(64, 40, 3, 1, 1, 1, 5, 7), _cv(32, 72, 3, 1, 1, 1, 5, 7, c1=64), _cv(64, 24, 4, 2, 1, 1, 9, 21)]   # slice-major
    # dual-source loader (channel counts not both multiples of 32) at the three widths
    t += [_cv(4, 8, 3, 1, 1, 1, 5, 7, c1=12), _cv(36, 40, 3, 1, 1, 1, 5, 7, c1=28), _cv(4, 72, 1, 1, 0, 2, 5, 7, c1=12),
          _cv(36, 130, 3, 1, 1, 1, 5, 7, c1=28, relu=True)]
    # scalar gather, each cause at some width: NCHW storage, C = 3 and 6, a pointer off by one float, a row stride % 4 != 0
    t += [_cv(8, 8, 3, 1, 1, 2, 5, 7, src0="nchw"), _cv(3, 40, 3, 1, 1, 1, 5, 7), _cv(6, 72, 3, 1, 1, 1, 5, 7),
          _cv(8, 33, 3, 1, 1, 1, 5, 7, src0="off1"), _cv(8, 130, 1, 1, 0, 1, 5, 7, src0="row"),
          _cv(8, 16, 3, 1, 1, 1, 5, 7, c1=8, src1="row"), _cv(64, 72, 3, 1, 1, 1, 5, 7, src0="nchw", mode=1)]
    # -- K edges, 1x1: K = 100 and 124 (tail), K = 64 and 96 (mode 1 takes them, mode 3 must not)
    t += [_cv(100, 40, 1, 1, 0, 1, 5, 7, mode=m) for m in (0, 1)] + [_cv(124, 72, 1, 1, 0, 1, 5, 7, mode=1)]
    t += [_cv(64, 192, 1, 1, 0, 2, 5, 7, mode=1), _cv(96, 40, 1, 1, 0, 1, 5, 7, mode=1), _cv(96, 40, 1, 1, 0, 1, 5, 7, mode=3),
          _cv(64, 16, 1, 1, 0, 1, 5, 7, mode=1)]
    # -- M edges (1x1 on 128 channels, mode 1 and exact): M = 1, 127, 128, 129; 7, 8 and 9 row tiles (the XCD remap's quotient
    # and remainder); a batch seam inside a tile (B = 3 x 50 pixels)
    for m in (0, 1):
        t += [_cv(128, 40, 1, 1, 0, 1, h, w, mode=m) for h, w in ((1, 1), (1, 127), (8, 16), (3, 43))]
        t += [_cv(32, 40, 3, 1, 1, 1, h, w, mode=m) for h, w in ((29, 29), (31, 33), (31, 37))]
        t += [_cv(32, 40, 3, 1, 1, 3, 5, 10, mode=m)]
    # -- geometry: pad 0, 1, 2 (pad 2: the input gradient of a 3x3 with padding 0); a map smaller than the kernel; stride 2 on odd maps
    t += [_cv(32, 40, 3, 1, p, 2, 5, 7, mode=m) for p in (0, 2) for m in (0, 1)]
    t += [_cv(32, 40, 3, 1, 1, 1, 1, 1, mode=1), _cv(32, 40, 4, 2, 1, 1, 2, 2, mode=1), _cv(32, 40, 4, 2, 1, 2, 9, 21, mode=1),
          _cv(8, 8, 4, 2, 1, 2, 9, 21)]
    # -- the split routes.  128x32: Cout <= 32, K >= 128, modes 1, 2, 3 (and 4: PREC 3, pieces unused)
    t += [_cv(32, 32, 3, 1, 1, 2, 5, 7, mode=m) for m in (1, 2, 3, 4)] + [_cv(128, 8, 1, 1, 0, 2, 5, 7, mode=1)]
    # Cout > 32 narrow in modes 1 .. 4 (wide: CONV_BIG_CASES for mode 1, below for 2 .. 4 through the four phases)
    t += [_cv(32, 72, 3, 1, 1, 2, 5, 7, mode=m) for m in (1, 2, 3, 4)] + [_cv(64, 64, 3, 1, 1, 2, 5, 7, mode=m, c1=32) for m in (1, 4)]
    # -- epilogues x tile widths x modes 0 and 1: no bias, ReLU, residual (NHWC and NCHW-strided), gates of both formats,
    # gate + residual (the input gradient of a residual block's 3x3)
    for m in (0, 1):
        for cout in (32, 64, 72):
            t += [_cv(32, cout, 3, 1, 1, 2, 5, 7, mode=m, bias=False, relu=True), _cv(32, cout, 3, 1, 1, 2, 5, 7, mode=m, res="nhwc", relu=True),
                  _cv(32, cout, 3, 1, 1, 2, 5, 7, mode=m, res="nchw", gate="f32", bias=False),
                  _cv(32, cout, 3, 1, 1, 2, 5, 7, mode=m, gate="pair", res="nhwc", bias=False)]
    t += [_cv(32, 130, 3, 1, 1, 2, 5, 7, mode=1, gate="f32"), _cv(8, 8, 3, 1, 1, 2, 5, 7, src0="nchw", gate="pair", res="nhwc")]
    # -- output layouts: NCHW through a direct call, a channel slice of a wider tensor (the gate laid out like it)
    t += [_cv(32, 40, 3, 1, 1, 2, 5, 7, mode=m, out="nchw") for m in (0, 1)]
    t += [_cv(32, 72, 3, 1, 1, 2, 5, 7, mode=1, out="slice", gate="f32"), _cv(32, 16, 3, 1, 1, 2, 5, 7, out="slice", res="nhwc"),
          _cv(32, 40, 3, 1, 1, 2, 5, 7, mode=1, src0="slice")]
    # -- mode 4 with pair formats, on shapes the LDS-DMA kernel does not take (128 <= K < 256 or Cout % 64 != 0) ...
    t += [_cv(128, 72, 1, 1, 0, 2, 5, 7, mode=4, pairs="0"), _cv(32, 64, 1, 1, 0, 2, 5, 7, mode=4, c1=96, pairs="1"),
          _cv(32, 72, 3, 1, 1, 2, 5, 7, mode=4, c1=32, pairs="01"), _cv(32, 72, 3, 1, 1, 2, 5, 7, mode=4, pairs="o", relu=True),
          _cv(128, 128, 1, 1, 0, 2, 5, 7, mode=4, pairs="0o")]
    # ... and on a shape it takes, with the kernel switched off; the same shape with it on is a hand-off
    t += [_cv(32, 64, 3, 1, 1, 2, 5, 7, mode=4, pairs="0o", knobs=(("ISI_NO_CONV_PAIR_KERNEL", 1),)),
          _cv(32, 64, 3, 1, 1, 2, 5, 7, mode=4, pairs="0o")]
    # -- silent downgrades: a split flag on a dual-source or gather launch runs exact fp32
    t += [_cv(36, 40, 3, 1, 1, 1, 5, 7, c1=28, mode=m) for m in (1, 2, 4)] + [_cv(6, 72, 3, 1, 1, 1, 5, 7, mode=m) for m in (1, 3)]
    # -- the four-phase launch: Cin 16 (K = 64: mode 1's route), 32, 48; Cout 5 (just beyond the few-channel kernel), 64, 96;
    # modes 0 .. 4; odd H and W; H = W = 1; NCHW output; gates of both formats; a pair-format source with the fused kernel off
    t += [_ct(16, 64, 2, 3, 5, mode=m) for m in (0, 1, 3)] + [_ct(32, 5, 2, 3, 5, mode=m) for m in (0, 1)]
    t += [_ct(32, 96, 2, 3, 5, mode=m) for m in (0, 1, 2, 3, 4)] + [_ct(48, 64, 1, 1, 1, mode=m) for m in (0, 1)]
    t += [_ct(32, 96, 1, 9, 21, mode=m, out="nchw", relu=True) for m in (0, 1)]
    t += [_ct(32, 64, 2, 3, 5, mode=1, gate="f32", bias=False), _ct(32, 64, 2, 3, 5, mode=0, gate="pair", bias=False),
          _ct(48, 96, 2, 3, 5, mode=1, gate="pair", bias=False), _ct(6, 8, 2, 3, 5, gate="f32"), _ct(8, 72, 1, 3, 5, src0="nchw")]
    t += [_ct(32, 64, 2, 3, 5, mode=4, pairs="0", knobs=(("ISI_NO_CONVT_PAIR_KERNEL", 1),)), _ct(32, 64, 2, 3, 5, mode=4, pairs="0"),
          _ct(32, 72, 2, 3, 5, mode=4, pairs="0o")]
    seen, out = set(), []
    for c in t:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


CONV_IGEMM_CASES = _conv_table() + CONV_BIG_CASES


def _conv_features(c):
    r = conv_route(c)
    f = set()
    if r <= 0:
        return {f"refused {r}"}
    R = conv_route_unpack(r)
    if R.family != 1:
        f.add(f"hand-off {CONV_FAMILIES[R.family]}")
        return f
    OH, OW = conv_out_hw(c)
    conv = c.op == "conv"
    M = c.B * (OH * OW if conv else c.H * c.W)
    Cin = c.c0 + c.c1
    K = (c.k * c.k if conv else 4) * Cin
    tiles = -(-M // CONV_BM)
    width = 32 if c.cout <= 32 else 64 if c.cout <= 64 else 128
    op = "conv" if conv else "four-phase"
    f |= {f"inst 128x{R.bn} {CONV_LOADERS[R.loader]} prec {R.prec} outp {R.outp}", f"{CONV_LOADERS[R.loader]} at Cout width {width}",
          f"{op}: prec {R.prec}", f"{op}: asked mode {c.mode}", f"M {M}", f"row tiles % 8 = {tiles % 8}" if tiles >= 7 else "few tiles",
          f"Cout {c.cout}", f"K {K} prec {R.prec}", f"{op}: out {c.out}"}
    if R.loader == 2:
        f |= {f"gather: {c.src0}" if c.src0 != "nhwc" else (f"gather: src1 {c.src1}" if c.c1 and c.src1 != "nhwc" else f"gather: C {c.c0}")}
    if R.prec and R.bn == 32:
        f.add(f"split 128x32 mode {c.mode}")
    if R.prec and R.bn > 32:
        t128 = tiles * -(-c.cout // 128) * (1 if conv else 4)
        f.add(f"split {'narrow' if R.bn == 64 else 'wide'} mode {c.mode}")
        if c.cout > 64:
            f.add(f"{op}: tiles128 {t128}")
    if c.mode and not R.prec:
        f.add(f"downgrade {CONV_LOADERS[R.loader]} mode {c.mode}" if R.loader else f"downgrade K {K} mode {c.mode}")
    if c.mode == 4 and R.prec == 3:
        f.add("mode 4 at Cout <= 32 runs prec 3")
    if K % 32:
        f.add(f"K tail {K}")
    if conv and R.loader == 0 and not R.slice_major and c.k > 1 and Cin % 32 and Cin > 32:
        f.add("chunk straddles taps")
    if R.slice_major:
        f.add(f"slice-major {'two sources' if c.c1 else 'k4 s2' if c.stride == 2 else 'one source'}" if conv else "slice-major four-phase")
    if conv:
        f.add(f"pad {c.pad}")
        if c.H < c.k and c.W < c.k:
            f.add(f"map smaller than the kernel k{c.k}")
        if c.stride == 2 and c.H % 2 and c.W % 2:
            f.add("stride 2 on an odd map")
        if c.B > 1 and (OH * OW) % CONV_BM:
            f.add("batch seam inside a tile")
        if c.src0 == "slice":
            f.add("source is a channel slice")
    else:
        f.add(f"four-phase: Cin {c.c0}")
        f.add(f"four-phase: Cout {c.cout}")
        if c.H % 2 and c.W % 2 and c.H > 1:
            f.add("four-phase: odd H and W")
        if c.H == 1 and c.W == 1:
            f.add("four-phase: H = W = 1")
    for p in c.pairs:
        f.add(f"{op}: pair {'output' if p == 'o' else 'source ' + p}")
    if c.pairs and c.knobs:
        f.add(f"{op}: pairs with {c.knobs[0][0]}")
    if "0" in c.pairs and "1" in c.pairs:
        f.add("conv: pair both sources")
    ep = f"{op} tile {R.bn} prec {min(R.prec, 1)}"          # (the tile the route runs, not the Cout class: 128 wide split = 640 tiles)
    if not c.bias:
        f.add(f"no bias: {ep}")
    if c.relu:
        f.add(f"relu: {ep}")
    if c.res:
        f.add(f"res {c.res}: {ep}")
    if c.gate:
        f.add(f"gate {c.gate}: {ep}")
        if c.res:
            f.add(f"gate + residual: {ep}")
        if c.out == "slice":
            f.add("gate on a sliced output")
    return f


def conv_igemm_requirements():
    """What CONV_IGEMM_CASES must reach (tests/test_conv_igemm_host.py asserts that nothing is missing)."""
    req = [f"inst 128x{bn} {ld} prec 0 outp 0" for bn in (32, 64, 128) for ld in CONV_LOADERS]
    req += [f"inst 128x{bn} uniform prec {p} outp 0" for bn in (32, 64, 128) for p in (1, 2, 3)]
    req += [f"inst 128x{bn} uniform prec 4 outp {o}" for bn in (64, 128) for o in (0, 1)]          # every instance launch_conv has
    req += [f"{ld} at Cout width {w}" for ld in CONV_LOADERS for w in (32, 64, 128)]
    req += ["gather: nchw", "gather: C 3", "gather: C 6", "gather: off1", "gather: row", "gather: src1 row"]
    req += [f"split 128x32 mode {m}" for m in (1, 2, 3)] + ["mode 4 at Cout <= 32 runs prec 3"]
    req += [f"split {nw} mode {m}" for nw in ("narrow", "wide") for m in (1, 2, 3, 4)]
    req += ["conv: pair source 0", "conv: pair source 1", "conv: pair both sources", "conv: pair output",
            "conv: pairs with ISI_NO_CONV_PAIR_KERNEL", "hand-off pair-dma"]
    req += ["K 64 prec 1", "K 96 prec 1", "K 96 prec 0", "downgrade K 96 mode 3", "K tail 36", "K tail 100", "K tail 124",
            "chunk straddles taps", "slice-major one source", "slice-major two sources", "slice-major k4 s2", "slice-major four-phase"]
    req += ["four-phase: tiles128 640", "conv: tiles128 639"]
    req += [f"M {m}" for m in (1, 127, 128, 129)] + [f"row tiles % 8 = {r}" for r in (7, 0, 1)] + ["batch seam inside a tile"]
    req += ["pad 0", "pad 1", "pad 2", "map smaller than the kernel k3", "map smaller than the kernel k4", "stride 2 on an odd map"]
    req += [f"Cout {n}" for n in (1, 33, 40, 72, 130)]
    for w in (32, 64, 128):
        for p in (0, 1):
            ep = f"conv tile {w} prec {p}"
            req += [f"no bias: {ep}", f"relu: {ep}", f"res nhwc: {ep}", f"res nchw: {ep}", f"gate f32: {ep}", f"gate pair: {ep}",
                    f"gate + residual: {ep}"]
    req += ["conv: out nhwc", "conv: out nchw", "conv: out slice", "four-phase: out nchw", "gate on a sliced output",
            "source is a channel slice"]
    req += [f"four-phase: Cin {n}" for n in (16, 32, 48)] + [f"four-phase: Cout {n}" for n in (5, 64, 96)]
    req += [f"four-phase: asked mode {m}" for m in range(5)] + [f"four-phase: prec {p}" for p in range(5)]
    req += ["four-phase: pair source 0", "four-phase: pairs with ISI_NO_CONVT_PAIR_KERNEL", "hand-off convT-pair", "four-phase: pair output",
            "gate f32: four-phase tile 64 prec 1", "gate pair: four-phase tile 64 prec 0", "gate pair: four-phase tile 64 prec 1",
            "gate pair: four-phase tile 128 prec 1",
            "four-phase: odd H and W", "four-phase: H = W = 1"]
    req += [f"downgrade dual mode {m}" for m in (1, 2, 4)] + [f"downgrade gather mode {m}" for m in (1, 3)]
    return req


def conv_hold(got, refs, prec, what, margin=ROW_OPS_MARGIN):
    """The comparison of the convolution tests: compare_rows per output channel against the spec, by the yardstick of the
    product mode `prec` the launch ran."""
    return compare_rows(conv_rows(got), conv_rows(refs.spec), conv_rows(conv_refs_yardstick(refs, prec)), what, margin)


CONV_FAKE_PTR = 0x10000        # non-null, 16-byte aligned, never dereferenced by a route query or a host-side refusal


def conv_lib_views(c, ptrs=None):
    """(src0, src1 or None, res or None, dst) ctypes views of a case over the storage addresses `ptrs` ({"src0", "src1",
    "res", "out": address of the storage's first float}; default: CONV_FAKE_PTR for all)."""
    from interactive_spectrogram_inpainting import _hip
    lay = conv_layout(c)
    at = lambda name: (ptrs or {}).get(name, CONV_FAKE_PTR) + 4 * lay[name].offset
    src = lambda name: _hip.isi_src(at(name), lay[name].shape[1], *lay[name].strides) if lay[name] else None
    return src("src0"), src("src1"), src("res"), _hip.isi_dst(at("out"), *lay["out"].strides)


def conv_lib_route(L, c, ptrs=None, mode=None, gate="case", pairs=None):
    """isi_conv2d_route / isi_conv_transpose2d_k4s2_route for a case (or the variant launch: another precision, gate or set
    of pair formats), under the case's knobs.  Launches nothing; with `ptrs` None no pointer is real."""
    import contextlib
    import ctypes as C
    from interactive_spectrogram_inpainting import _hip
    s0, s1, res, dst = conv_lib_views(c, ptrs)
    at = lambda name: (ptrs or {}).get(name, CONV_FAKE_PTR)
    ref = lambda v: C.byref(v) if v is not None else None
    gate_kind = c.gate if gate == "case" else gate
    g = at("gate") + 4 * conv_layout(c)["out"].offset if gate_kind else None
    flags = conv_case_flags(c, mode, gate, pairs)
    with contextlib.ExitStack() as stack:
        for name, value in c.knobs:
            stack.enter_context(_hip.knob(name, value))
        if c.op == "convT":
            return L.isi_conv_transpose2d_k4s2_route(ref(s0), at("w"), at("bias") if c.bias else None, g, ref(dst), c.B, c.H, c.W,
                                                     c.cout, flags)
        return L.isi_conv2d_route(ref(s0), ref(s1), at("w"), at("bias") if c.bias else None, ref(res), g, ref(dst), c.B, c.H, c.W,
                                  c.cout, c.k, c.k, c.stride, c.pad, flags)


def conv_igemm_coverage_gaps(cases):
    """The requirements above that no case of `cases` reaches."""
    have = set()
    for c in cases:
        have |= _conv_features(c)
    return [r for r in conv_igemm_requirements() if r not in have]
