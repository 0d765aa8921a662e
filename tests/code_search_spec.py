"""Specification of the code-database search (csrc/code_search.hip), shared by the host and the
GPU tests.  For one layer with codebook E [K, D], query q [C], stored map x [C] and cell weights w [C] >= 0:

    T[a][b]    = sum_d (E[a][d] - E[b][d])^2
    dist(q, x) = sum_c w[c] T[q[c]][x[c]]            cells with q[c] >= K (the priors' mask token) count nothing

`table64` / `search64` evaluate the two in float64 from the SAME fp32 inputs the kernels read (the fp32 codebook; the fp32
table and weights); `search_int` is the exact int64 form for integer tables and 0/1 weights.  The bounds are derived, not
measured (u = 2^-24, the unit roundoff of fp32):

  table   each difference is rounded once (relative u, so its square carries 2u), and the fma chain rounds once per
          step: a term passes through at most D roundings.  All terms are >= 0, so |T - T64| <= ((1 + u)^(D + 2) - 1) T64
          <= (D + 4) u T64 for every D this project can meet (D <= 2^11).
  search  each product w T is rounded once; the products of a run of 256 consecutive cells are added in cell order (the
          first one to 0, exactly), the run sums in run order: a term passes through at most 1 + 255 + ceil(C / 256) - 1
          <= C + 1 roundings, so |dist - spec| <= ((1 + u)^(C + 1) - 1) S <= (C + 2) u S with S = sum_c |w[c] T[..]|, for
          C <= 5792 by the bare count and for every C the kernel takes by the run structure (256 + C / 256 roundings).
          Integer tables, weights 0 or 1 and sums below 2^24: every operation is exact.

`emulate_f32` is the kernel's arithmetic on the host in IEEE fp32 (numpy), for the tests that need no device."""
import numpy as np

U = 2.0 ** -24
RUN = 256          # cells per sequential run (csrc/code_search.hip: CS_SPLIT)
FAKE = 0x10000     # non-null, 16-byte aligned, never dereferenced on the host


def table64(codebook32):
    """codebook [K, D] fp32 -> T [K, K] float64."""
    e = np.asarray(codebook32, dtype=np.float32).astype(np.float64)
    out = np.empty((e.shape[0], e.shape[0]))
    for a0 in range(0, e.shape[0], 64):                               # (row blocks: the [K, K, D] cube stays small)
        diff = e[a0:a0 + 64, None, :] - e[None, :, :]
        out[a0:a0 + 64] = (diff * diff).sum(-1)
    return out


def table_bound(t64, D):
    return (D + 4) * U * t64


def _terms(codes, q, w, table, dtype):
    """[N, C] of w[c] T[q[c]][x[c]] in `dtype` arithmetic (one rounding per product), zeros where q[c] >= K."""
    table = np.asarray(table)
    K = table.shape[0]
    codes = np.asarray(codes).astype(np.int64)
    q = np.asarray(q).astype(np.int64)
    C = q.shape[0]
    live = q < K
    rows = table[np.where(live, q, 0)].astype(dtype)                 # [C, K]
    vals = rows[np.arange(C)[None, :], codes]                        # [N, C]
    weight = np.ones(C, dtype) if w is None else np.asarray(w).astype(dtype)
    return np.where(live[None, :], vals * weight[None, :], dtype(0))


def search64(codes, query, weights, table32):
    """codes [N, C], query [Q, C], weights [Q, C] fp32 or None, table [K, K] fp32 -> (dist [Q, N], S [Q, N]) float64,
    S = sum_c |w[c] T[..]| (what the bound scales with)."""
    query = np.asarray(query)
    dist, mag = [], []
    for j in range(query.shape[0]):
        t = _terms(codes, query[j], None if weights is None else np.asarray(weights, dtype=np.float32)[j],
                   np.asarray(table32, dtype=np.float32), np.float64)
        dist.append(t.sum(1))
        mag.append(np.abs(t).sum(1))
    return np.stack(dist), np.stack(mag)


def search_int(codes, query, weights01, table_int):
    """The exact form: integer table, weights in {0, 1} (or None) -> int64 [Q, N]."""
    query = np.asarray(query)
    out = []
    for j in range(query.shape[0]):
        w = None if weights01 is None else np.asarray(weights01)[j].astype(np.int64)
        out.append(_terms(codes, query[j], w, np.asarray(table_int).astype(np.int64), np.int64).sum(1))
    return np.stack(out)


def search_bound(mag, C):
    return (C + 2) * U * mag


def emulate_f32(codes, query, weights, table32):
    """The kernel's arithmetic in IEEE fp32: products rounded once, runs of RUN cells added in cell order from 0, the
    run sums added in run order."""
    query = np.asarray(query)
    out = []
    for j in range(query.shape[0]):
        t = _terms(codes, query[j], None if weights is None else np.asarray(weights, dtype=np.float32)[j],
                   np.asarray(table32, dtype=np.float32), np.float32)
        total = None
        for c0 in range(0, t.shape[1], RUN):
            acc = np.zeros(t.shape[0], np.float32)
            for c in range(c0, min(c0 + RUN, t.shape[1])):
                acc = acc + t[:, c]
            total = acc if total is None else total + acc
        out.append(total)
    return np.stack(out)


def apply_allowed(dist, allowed):
    """Items with allowed[n] == 0 get +inf."""
    out = np.array(dist, dtype=np.float64, copy=True)
    if allowed is not None:
        out[:, np.asarray(allowed) == 0] = np.inf
    return out
