"""Specification of the code-database search by encoder vectors (csrc/code_search.hip, csrc/code_shift_search.hip;
DESIGN.md section 6c.2), shared by the host and the GPU tests.  It builds on tests/code_search_spec.py (`S`) and
tests/code_shift_search_spec.py (`SH`) and changes neither.

The layer has the codebook E [K, D]; a query has per-cell vectors z [cells, D] and the search sees them as ROWS:

    R[c][k]    = sum_d (z[c][d] - E[k][d])^2             fp32, d ascending, one fma per d: the table's expression (S.table64)
    dist[j][n] = sum_c w[j][c] R[j][c][codes[n][c]]      a cell whose weight is exactly 0 contributes +0 whatever R holds

  contract 1  where z[c] is codebook row a bit for bit, R[c][:] is T[a][:] bit for bit
  contract 2  with R[j][c] = T[query[j][c]] gathered by the caller (mask-token cells under weight 0) dist is
              isi_code_search_f32's, bit for bit
  contract 3  the shifted rows search with gathered table rows is isi_code_shift_search_f32's, bit for bit
  contract 4  the shifted rows search at W == T, S == 1, shift0 == 0 is the aligned rows search, bit for bit

Bounds (u = 2^-24), by the derivations of tests/code_search_spec.py -- the rows are the table's sum with another left
operand, the search is the hard search's sum with another staged row:

  rows    |R - R64| <= (D + 4) u R64
  search  |dist - spec| <= (C + 2) u sum_c |w[c] R[..]|; exact for integer rows, weights 0 or 1 and sums below 2^24

A stored code >= K is clamped to K - 1.  `rows64` / `search64` evaluate in float64 from the fp32 inputs the kernels read,
`search_int` is the exact int64 form, `rows_emulate_f32` / `emulate_f32` are the kernels' arithmetic in IEEE fp32."""
import numpy as np

import code_search_spec as S
import code_shift_search_spec as SH

U, RUN, FAKE = S.U, S.RUN, S.FAKE


def rows64(z32, codebook32):
    """z [cells, D] fp32, codebook [K, D] fp32 -> R [cells, K] float64."""
    z = np.asarray(z32, dtype=np.float32).astype(np.float64)
    e = np.asarray(codebook32, dtype=np.float32).astype(np.float64)
    out = np.empty((z.shape[0], e.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, z.shape[0], 64):                            # (cell blocks: the [cells, K, D] cube stays small)
            diff = z[c0:c0 + 64, None, :] - e[None, :, :]
            out[c0:c0 + 64] = (diff * diff).sum(-1)
    return out


def rows_bound(r64, D):
    return S.table_bound(r64, D)


def rows_emulate_f32(z32, codebook32):
    """The rows kernel's arithmetic (and, with z = the codebook, the table kernel's): the difference rounded to fp32, then
    acc = fma(diff, diff, acc) with d ascending.  The fma is the float64 sum of the exact 48-bit square and the
    accumulator, rounded to fp32 (tests/test_code_search_host.py's form of it): one rounding wherever that float64 sum is
    exact, which the bound checks do not depend on and the bitwise checks -- emulation against emulation -- cannot see."""
    z = np.asarray(z32, dtype=np.float32)
    e = np.asarray(codebook32, dtype=np.float32)
    acc = np.zeros((z.shape[0], e.shape[0]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(e.shape[1]):
            diff = (z[:, None, d] - e[None, :, d]).astype(np.float32)
            acc = (diff.astype(np.float64) * diff.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def gather_rows(table, query):
    """Contract 2's rows: R[j][c] = T[query[j][c]] -> [Q, C, K] in the table's type.  A mask-token cell (query >= K) has
    no table row: it gets row 0 and must be given weight 0 (`mask_token_weights`)."""
    table = np.asarray(table)
    query = np.asarray(query).astype(np.int64)
    return table[np.where(query < table.shape[0], query, 0)]


def mask_token_weights(query, weights, K):
    """weights [Q, C] fp32 (None: ones) with 0 on the mask-token cells -- what both searches of contract 2 are given."""
    query = np.asarray(query)
    w = np.ones(query.shape, np.float32) if weights is None else np.array(weights, dtype=np.float32, copy=True)
    w[query >= K] = 0
    return w


def _terms(codes, rows, w, dtype):
    """[N, C] of w[c] R[c][x[c]] in `dtype` arithmetic (one rounding per product), +0 where w[c] == 0."""
    rows = np.asarray(rows)
    C, K = rows.shape
    codes = np.minimum(np.asarray(codes).astype(np.int64), K - 1)    # a stored code >= K is clamped
    vals = rows.astype(dtype)[np.arange(C)[None, :], codes]           # [N, C]
    if w is None:
        return vals
    weight = np.asarray(w).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where((weight == 0)[None, :], dtype(0), vals * weight[None, :])


def _w(weights, j):
    return None if weights is None else np.asarray(weights, dtype=np.float32)[j]


def search64(codes, rows32, weights):
    """codes [N, C], rows [Q, C, K] fp32, weights [Q, C] fp32 or None -> (dist [Q, N], mag [Q, N]) float64,
    mag = sum_c |w[c] R[..]| (what the bound scales with)."""
    rows32 = np.asarray(rows32, dtype=np.float32)
    dist, mag = [], []
    for j in range(rows32.shape[0]):
        t = _terms(codes, rows32[j], _w(weights, j), np.float64)
        dist.append(t.sum(1))
        mag.append(np.abs(t).sum(1))
    return np.stack(dist), np.stack(mag)


def search_int(codes, rows_int, weights01):
    """The exact form: integer rows, weights in {0, 1} (or None) -> int64 [Q, N]."""
    rows_int = np.asarray(rows_int)
    out = []
    for j in range(rows_int.shape[0]):
        w = None if weights01 is None else np.asarray(weights01)[j].astype(np.int64)
        out.append(_terms(codes, rows_int[j].astype(np.int64), w, np.int64).sum(1))
    return np.stack(out)


def search_bound(mag, C):
    return S.search_bound(mag, C)


def emulate_f32(codes, rows32, weights):
    """The kernel's arithmetic in IEEE fp32: products rounded once, runs of RUN cells added in cell order from 0, the run
    sums added in run order."""
    rows32 = np.asarray(rows32, dtype=np.float32)
    out = []
    for j in range(rows32.shape[0]):
        t = _terms(codes, rows32[j], _w(weights, j), np.float32)
        total = None
        with np.errstate(invalid="ignore", over="ignore"):
            for c0 in range(0, t.shape[1], RUN):
                acc = np.zeros(t.shape[0], np.float32)
                for c in range(c0, min(c0 + RUN, t.shape[1])):
                    acc = acc + t[:, c]
                total = acc if total is None else total + acc
        out.append(total)
    return np.stack(out)


apply_allowed = S.apply_allowed


# ---- the shifted search: window rows [Q, F * W, K] (cell c = f * W + t) over stored maps codes [N, F, T].  One offset o IS
# the aligned rows search on the cropped maps codes[:, :, o:o + W] flattened to [N, F * W] (SH.crop).
def _per_offset(fn, codes, rows, weights, W, shift0, step, count):
    weights = None if weights is None else np.asarray(weights).reshape(np.asarray(weights).shape[0], -1)
    return [fn(SH.crop(codes, o, W), rows, weights) for o in SH.offsets(shift0, step, count)]


def shift_search64(codes, rows32, weights, W, shift0, step, count):
    """-> (dist [Q, S, N], mag [Q, S, N]) float64."""
    per = _per_offset(search64, codes, rows32, weights, W, shift0, step, count)
    return np.stack([p[0] for p in per], 1), np.stack([p[1] for p in per], 1)


def shift_search_int(codes, rows_int, weights01, W, shift0, step, count):
    """The exact form -> int64 [Q, S, N]."""
    return np.stack(_per_offset(search_int, codes, rows_int, weights01, W, shift0, step, count), 1)


def shift_emulate(codes, rows32, weights, W, shift0, step, count):
    """The kernel's arithmetic in IEEE fp32 -> float32 [Q, S, N]."""
    return np.stack(_per_offset(emulate_f32, codes, rows32, weights, W, shift0, step, count), 1)


def shift_bound(mag, F, W):
    return S.search_bound(mag, F * W)
