"""Specification of the shift-invariant code search (csrc/code_shift_search.hip), shared by the
host and the GPU tests.  Stored maps codes [N, F, T], query windows query [Q, F, W] with W <= T, cell weights
weights [Q, F, W] >= 0 or None, table T_ [K, K]; offsets o_s = shift0 + s * step, s = 0 .. S-1, each with o_s + W <= T:

    dist[j][s][n] = sum_f sum_t w[j][f][t] T_[query[j][f][t]][codes[n][f][t + o_s]]     query cells >= K count nothing

The specification for one offset o IS the aligned search of tests/code_search_spec.py applied to the cropped maps
codes[:, :, o:o + W] flattened to [N, F * W]: the same products, the same cell numbering c = f * W + t, the same runs of
256 cells, so the same bound with C = F * W, |dist - spec| <= (F W + 2) u sum |w T_[..]|, and the same exactness for
integer tables.  best[j][n] = min_s dist[j][s][n]; best_shift[j][n] the smallest s attaining it (int32); +inf and -1
where allowed[n] == 0."""
import numpy as np

import code_search_spec as S

U, RUN, FAKE = S.U, S.RUN, S.FAKE


def offsets(shift0, step, count):
    return [shift0 + s * step for s in range(count)]


def crop(codes, o, W):
    """codes [N, F, T] -> the columns [o, o + W) flattened to [N, F * W]."""
    codes = np.asarray(codes)
    N, F, T = codes.shape
    assert 0 <= o and o + W <= T
    return np.ascontiguousarray(codes[:, :, o:o + W]).reshape(N, F * W)


def _flat(a):
    return None if a is None else np.asarray(a).reshape(np.asarray(a).shape[0], -1)


def _per_offset(fn, codes, query, weights, table, shift0, step, count):
    W = np.asarray(query).shape[2]
    return [fn(crop(codes, o, W), _flat(query), _flat(weights), table) for o in offsets(shift0, step, count)]


def search64(codes, query, weights, table32, shift0, step, count):
    """-> (dist [Q, S, N], mag [Q, S, N]) float64; mag = sum |w T_[..]|, what the bound scales with."""
    per = _per_offset(S.search64, codes, query, weights, table32, shift0, step, count)
    return np.stack([p[0] for p in per], 1), np.stack([p[1] for p in per], 1)


def search_int(codes, query, weights01, table_int, shift0, step, count):
    """The exact form -> int64 [Q, S, N]."""
    return np.stack(_per_offset(S.search_int, codes, query, weights01, table_int, shift0, step, count), 1)


def emulate(codes, query, weights, table32, shift0, step, count):
    """The kernel's arithmetic in IEEE fp32 -> float32 [Q, S, N]."""
    return np.stack(_per_offset(S.emulate_f32, codes, query, weights, table32, shift0, step, count), 1)


def bound(mag, F, W):
    return S.search_bound(mag, F * W)


def best(dist, allowed=None):
    """dist [Q, S, N] -> (best [Q, N] in dist's type widened to float64, best_shift int32 [Q, N])."""
    dist = np.asarray(dist)
    shift = np.argmin(dist, axis=1).astype(np.int32)                  # (numpy: the first of equal minima)
    value = np.take_along_axis(dist, shift[:, None, :].astype(np.int64), 1)[:, 0, :].astype(np.float64)
    if allowed is not None:
        off = np.asarray(allowed) == 0
        value[:, off] = np.inf
        shift[:, off] = -1
    return value, shift
