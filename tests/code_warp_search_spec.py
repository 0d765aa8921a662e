"""Specification of the time-warped code search (csrc/code_warp_search.hip), shared by the host
and the GPU tests.  It changes none of the other specifications.

A grid has W query columns and T item columns.  The query is one or two PARTS (a top layer, a bottom layer, or both); part p
has F_p rows, r_p >= 1 columns of its own per grid column, stored codes codes_p [N, F_p, T r_p], per-cell cost rows
rows_p [Q, F_p * W r_p, K_p] (cell c = f * (W r_p) + (i r_p + u)) and weights w_p [Q, F_p, W r_p] >= 0 or None.

    cost[i][t] = sum_p sum_f sum_u  fl( w_p[f][i r_p + u] * rows_p[c][x] ),     x = min(codes_p[n][f][t r_p + u], K_p - 1)

in fp32 from +0, each product rounded once, added in the order parts, f ascending, u ascending; a cell whose weight is
exactly 0 adds +0 whatever its row holds.  Query column i is matched to item column p(i) with p(i+1) - p(i) in {0, 1, 2}
(hold, step, skip), lo <= p(i) - i <= hi and 0 <= p(i) <= T - 1:

    D[0][t] = cost[0][t]                                                          (admissible t)
    D[i][t] = fl( cost[i][t] + min(D[i-1][t-1], D[i-1][t], D[i-1][t-2]) )         (+inf where (i, t) is not admissible)
    dist    = min_t D[W-1][t],  end = the smallest t that attains it;  +inf and -1 without a path or where allowed[n] == 0

`min` is taken by strict comparisons in the order t-1, t, t-2 (a later candidate wins only if it is smaller): that is the
tie rule of the path, and it says what a NaN does.  fp32 min is exact and fp32 addition is monotone, so dist is the minimum
over all admissible paths of the path's left-to-right fp32 sum; the tie rule changes the path, never the distance.

Bound (u = 2^-24), for rows >= 0 under non-zero weight.  A column cost is a sum of V = sum_p F_p r_p rounded products:
cost = cost64 (1 + d) with |d| <= (1 + u)^V - 1.  Along one path the W costs are added left to right, W - 1 roundings,
so that path's fp32 sum is within (1 + u)^(V + W - 1) - 1 of its float64 sum, relatively -- all terms are >= 0.  The
minimum over paths of values each within a relative e of its exact value is within e of the exact minimum.  With
(1 + u)^n - 1 <= n u / (1 - n u) and n <= 2^12:  |dist - dist64| <= (V + W + 2) u dist64.

`steps` (the predecessors in order of preference, as p(i) - p(i-1)) exists for the planted-fault tests only."""
import numpy as np

U = 2.0 ** -24
STEPS = (1, 0, 2)
INT_INF = 1 << 60


class Part:
    """One layer of a warped query against the stored maps of that layer."""

    def __init__(self, codes, rows, weights=None, r=1):
        self.codes = np.asarray(codes)
        self.rows = np.asarray(rows)
        self.weights = None if weights is None else np.asarray(weights)
        self.r = int(r)
        N, F, Tr = self.codes.shape
        assert Tr % self.r == 0 and self.rows.shape[1] % (F * self.r) == 0
        self.N, self.F, self.T, self.K = N, F, Tr // self.r, self.rows.shape[2]
        self.Q, self.W = self.rows.shape[0], self.rows.shape[1] // (F * self.r)

    def products(self):
        return self.F * self.r


def grid(parts):
    """(N, T, W, Q, V) of a list of parts (they must agree)."""
    first = parts[0]
    assert all((p.N, p.T, p.W, p.Q) == (first.N, first.T, first.W, first.Q) for p in parts)
    return first.N, first.T, first.W, first.Q, sum(p.products() for p in parts)


def column_cost(parts, j, dtype):
    """cost [N, W, T] of query j in `dtype` arithmetic (np.float32: the kernel's; np.float64; np.int64)."""
    N, T, W, _, _ = grid(parts)
    cost = np.zeros((N, W, T), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in parts:
            rows = p.rows[j].reshape(p.F, W * p.r, p.K)
            weights = None if p.weights is None else p.weights[j].reshape(p.F, W * p.r)
            codes = np.minimum(p.codes.astype(np.int64), p.K - 1)      # a stored code >= K is clamped
            for f in range(p.F):
                for u in range(p.r):
                    vals = rows[f, u::p.r].astype(dtype)[:, codes[:, f, u::p.r]].transpose(1, 0, 2)     # [N, W, T]
                    if weights is not None:
                        w = weights[f, u::p.r].astype(dtype)[None, :, None]
                        vals = np.where(w == 0, dtype(0), vals * w)
                    cost = cost + vals
    return cost


def admissible(W, T, lo, hi):
    """bool [W, T]: 0 <= t <= T - 1 and lo <= t - i <= hi."""
    drift = np.arange(T)[None, :] - np.arange(W)[:, None]
    return (drift >= lo) & (drift <= hi)


def align(cost, lo, hi, steps=STEPS):
    """The recurrence on cost [N, W, T] in cost's type -> (dist [N], end int32 [N], back int8 [N, W, T]: the chosen
    p(i) - p(i-1), -1 where there is none).  Integer costs use INT_INF for +inf."""
    cost = np.asarray(cost)
    N, W, T = cost.shape
    integer = cost.dtype.kind == "i"
    inf = cost.dtype.type(INT_INF) if integer else cost.dtype.type(np.inf)
    ok = admissible(W, T, lo, hi)
    back = np.full((N, W, T), -1, np.int8)
    D = np.where(ok[0][None, :], cost[:, 0], inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, W):
            best = np.full((N, T), inf, cost.dtype)
            pick = np.full((N, T), -1, np.int8)
            for k, step in enumerate(steps):
                cand = np.full((N, T), inf, cost.dtype)
                cand[:, step:] = D[:, :T - step] if step else D
                take = (cand < best) if k else np.ones((N, T), bool)
                best = np.where(take, cand, best)
                pick = np.where(take, np.int8(step), pick)
            total = cost[:, i] + best
            if integer:
                total = np.where(best >= inf, inf, total)
            D = np.where(ok[i][None, :], total, inf)
            back[:, i] = np.where(ok[i][None, :], pick, -1)
    dist = np.full(N, inf, cost.dtype)
    end = np.full(N, -1, np.int32)
    for t in range(T):                                                 # strict: the smallest t among equal minima
        take = D[:, t] < dist
        dist = np.where(take, D[:, t], dist)
        end = np.where(take, np.int32(t), end)
    return dist, end, back


def backtrack(end, back):
    """path int32 [N, W]: p(i) from `end` through the back-pointers; -1 throughout where end == -1."""
    N, W, _ = back.shape
    path = np.full((N, W), -1, np.int32)
    for n in range(N):
        t = int(end[n])
        if t < 0:
            continue
        for i in range(W - 1, -1, -1):
            path[n, i] = t
            if i:
                t -= int(back[n, i, t])
    return path


def _search(parts, lo, hi, dtype, allowed, steps):
    N, _, _, Q, _ = grid(parts)
    dist, end, path = [], [], []
    for j in range(Q):
        d, e, back = align(column_cost(parts, j, dtype), lo, hi, steps)
        if allowed is not None:
            off = np.asarray(allowed) == 0
            d = np.where(off, d.dtype.type(INT_INF if d.dtype.kind == "i" else np.inf), d)
            e = np.where(off, np.int32(-1), e)
        dist.append(d)
        end.append(e)
        path.append(backtrack(e, back))
    return np.stack(dist), np.stack(end), np.stack(path)


def emulate(parts, lo, hi, allowed=None, steps=STEPS):
    """The kernel's arithmetic in IEEE fp32 -> (dist float32 [Q, N], end int32 [Q, N], path int32 [Q, N, W])."""
    return _search(parts, lo, hi, np.float32, allowed, steps)


def search64(parts, lo, hi, allowed=None):
    """The same recurrence in float64 on the same fp32 factors -> dist float64 [Q, N]."""
    return _search(parts, lo, hi, np.float64, allowed, STEPS)[0]


def search_int(parts, lo, hi, allowed=None, steps=STEPS):
    """The exact form (integer rows, weights 0 or 1) -> (dist int64 [Q, N] with INT_INF for +inf, end, path)."""
    return _search(parts, lo, hi, np.int64, allowed, steps)


def bound(dist64, parts):
    _, _, W, _, V = grid(parts)
    return (V + W + 2) * U * np.asarray(dist64, dtype=np.float64)


def has_path(W, T, lo, hi):
    """Whether the first and the last query column have an admissible cell (then a path exists: drift is kept by `step`)."""
    ok = admissible(W, T, lo, hi)
    return bool(ok[0].any() and ok[W - 1].any())


def path_admissible(path, T, lo, hi):
    """Whether path [W] (item columns) keeps the steps, the band and the item's ends."""
    path = np.asarray(path).astype(np.int64)
    drift = path - np.arange(len(path))
    steps = np.diff(path)
    return bool((path >= 0).all() and (path <= T - 1).all() and (drift >= lo).all() and (drift <= hi).all()
                and ((steps >= 0) & (steps <= 2)).all())


def brute_force(cost, lo, hi):
    """Every admissible path of one item's cost [W, T], enumerated: (the least left-to-right sum in cost's type, or None)."""
    cost = np.asarray(cost)
    W, T = cost.shape
    ok = admissible(W, T, lo, hi)
    best = [None]

    def walk(i, t, total):
        if not ok[i, t]:
            return
        with np.errstate(invalid="ignore", over="ignore"):
            total = cost[i, t] if i == 0 else cost[i, t] + total       # (numpy scalars of cost's type: one rounding)
        if i == W - 1:
            if best[0] is None or total < best[0]:
                best[0] = total
            return
        for step in (0, 1, 2):
            if t + step < T:
                walk(i + 1, t + step, total)
    for t in range(T):
        walk(0, t, None)
    return best[0]
