"""Float64 specification of the top-M / palette-restricted codebook search (csrc/vq_topm.hip, isi_vq_nearest_topm_f32), the
test data of its host and GPU tests, an fp32 model of the kernel with planted faults, and the comparison both test files
use.  CPU only.

For N vectors z [N, D], a codebook E [K, D], palettes `allowed` bool [P, K] (None: every code) and a palette row per vector
`allowed_row` [N] (None: row 0):

    d[n, k]  = |z_n|^2 - 2 z_n.e_k + |e_k|^2
    rank m   = the m-th smallest (d, k) pair in lexicographic order over the codes k that the vector's palette allows and
               whose distance is < +inf                                              (ties: the lower code first)

* Identical code vectors have identical distances by definition (the spec computes one distance per distinct row).
* A palette with fewer than M such codes: the missing ranks are id -1, distance +inf.  A row outside [0, P): empty palette.
* A vector with a non-finite component: id -1, distance NaN at every rank.
* A code vector with a non-finite component is never returned and changes nothing else.

Two inequalities tie the fp32 kernel to this.  u = 2^-24; S(n, k) = |z|^2 + 2 sum_i |z_i e_ki| + |e_k|^2.

DISTANCE.  |d - d64| <= (D + 3) u S (1 + 2^-20).  The kernel computes fl(fl(x2 - 2 dot) + e2) with x2, dot and e2 each a
D-term fp32 sum of products.  A D-term sum of products rounded once per term (product and addition fused or not, in any
order) errs by at most D u times the sum of the terms' magnitudes, up to O(u^2): D u |z|^2 for x2, D u sum|z_i e_ki| for
dot -- doubled exactly by the factor 2 -- and D u |e_k|^2 for e2 (isi_pack_codebook_f32's sum).  The two roundings of the
association err by u |x2 - 2 dot| and u |d|, both at most u S, and the exchange of the two half-sums of x2 is one of its D
additions.  Total (D + 2) u S + O(u^2) <= (D + 3) u S.  The matrix pipe's accumulation (v_mfma_f32_32x32x2f32: two
products per instruction added into the fp32 accumulator) rounds at most once per product, which is what the D-term bound
assumes; no wider constant is needed, and the GPU test measures the worst ratio it meets.

ORDER.  x2 is one number for all codes of a vector, so its error moves every distance of the vector alike -- up to the
association's two roundings -- and does not reorder them.  What can reorder codes a and b is the error of -2 dot + e2 and
the association: at most (D + 2) u (2 sum|z_i e_i| + |e|^2) + 2 u S <= 2 (D + 4) u (|z|^2 + |e|^2) per code (2 |z.e| <=
|z|^2 + |e|^2).  In the worst case -- every rounding aligned -- the order is guaranteed from a normalised gap
(d64_b - d64_a) / (|z|^2 + |e_a|^2) of about 4 (D + 4) u: 1.6e-5 at D = 64, 3e-6 at D = 8.  Roundings do not align: they
accumulate like a random walk, sqrt(D) instead of D, which puts the typical error of a D = 64 distance at 1e-6 of
|z|^2 + |e|^2 -- the reason the project certifies a moved index below 2e-6 and calls data with gaps of at least
MIN_GAP = 1e-5 near-tie free (oracle.near_tie_free_vectors, tests/golden/quantizer_large.npz).  This file follows that
convention: on vectors whose consecutive float64 gaps among the nine nearest allowed codes are all >= MIN_GAP the
kernel's ids must equal the spec's exactly; elsewhere a differing id must be a certified near-tie, gap < CERTIFY.
"""
from types import SimpleNamespace

import torch

MIN_GAP = 1e-5
CERTIFY = 2e-6
MAX_REJECTED = 0.02
GAP_RANKS = 9
ID_POISON = 0x5A5A5A5A5A5A5A5A
DIST_POISON = 0x7FC12345        # a NaN no kernel produces
U = 2.0 ** -24


# --------------------------------------------------------------------------------------------------- the specification
def distances64(z, E):
    """d64 [N, K] float64, one distance per DISTINCT code row; +inf for a code with a non-finite component; NaN rows for a
    vector with a non-finite component.  Also the bound's magnitude S [N, K]."""
    zd, Ed = z.double(), E.double()
    uniq, inverse = torch.unique(Ed, dim=0, return_inverse=True)
    good = torch.isfinite(uniq).all(1)
    clean = torch.where(good[:, None], uniq, torch.zeros_like(uniq))
    lost = ~torch.isfinite(zd).all(1)
    zc = torch.where(lost[:, None], torch.zeros_like(zd), zd)
    x2, e2 = zc.pow(2).sum(1, keepdim=True), clean.pow(2).sum(1)
    d = x2 - 2 * zc @ clean.T + e2
    S = x2 + 2 * zc.abs() @ clean.abs().T + e2
    d[:, ~good] = float("inf")
    d, S = d[:, inverse], S[:, inverse]
    d[lost] = float("nan")
    return d, S, x2[:, 0], (Ed.pow(2).sum(1))


def allowed_matrix(N, K, allowed, allowed_row):
    """bool [N, K]: the codes each vector may receive"""
    if allowed is None:
        return torch.ones(N, K, dtype=torch.bool)
    P = allowed.shape[0]
    row = torch.zeros(N, dtype=torch.int64) if allowed_row is None else allowed_row.long()
    inside = (row >= 0) & (row < P)
    return allowed[torch.where(inside, row, torch.zeros_like(row))] & inside[:, None]


def topm_spec(z, E, M, allowed=None, allowed_row=None):
    """-> ids int64 [M, N], dist float64 [M, N] by the module's docstring."""
    N, K = z.shape[0], E.shape[0]
    d, _, _, _ = distances64(z, E)
    lost = torch.isnan(d).any(1)
    masked = torch.where(allowed_matrix(N, K, allowed, allowed_row), d, torch.full_like(d, float("inf")))
    masked[lost] = float("inf")
    order = torch.sort(masked, dim=1, stable=True)        # stable: equal distances keep the lower code in front
    m = min(M, K)
    dist = torch.full((M, N), float("inf"), dtype=torch.float64)
    ids = torch.full((M, N), -1, dtype=torch.int64)
    dist[:m], ids[:m] = order.values[:, :m].T, order.indices[:, :m].T
    ids[dist == float("inf")] = -1
    dist[:, lost] = float("nan")
    return ids, dist


def near_tie_free(z, E, allowed=None, allowed_row=None, ranks=GAP_RANKS, min_gap=MIN_GAP):
    """bool [N]: every consecutive float64 gap among the vector's `ranks` nearest allowed codes, normalised by
    |z|^2 + |e|^2 of the nearer one, is at least min_gap (ranks that do not exist make no gap).  Two IDENTICAL code
    vectors at consecutive ranks are no near-tie: their distances are equal by definition -- and bit for bit in any
    implementation that computes both the same way -- so the index rule alone orders them."""
    ids, dist = topm_spec(z, E, ranks, allowed, allowed_row)
    _, _, x2, e2 = distances64(z, E)
    e2 = torch.where(torch.isfinite(e2), e2, torch.zeros_like(e2))
    exists = ids >= 0
    scale = x2[None, :] + e2[ids.clamp(min=0)]
    same_row = torch.unique(E.double(), dim=0, return_inverse=True)[1][ids.clamp(min=0)]
    pair = exists[:-1] & exists[1:] & (same_row[:-1] != same_row[1:])
    gap = torch.where(pair, (dist[1:] - dist[:-1]) / scale[:-1], torch.full_like(scale[:-1], float("inf")))
    return (gap >= min_gap).all(0)


# ------------------------------------------------------------------------------------------------------- the test data
def duplicate_pairs(K):
    return [(1, K // 2 + 5), (K // 3, K - 1)]


def make_case(N, D, K, seed=0, palettes=True, pad=(3, 5)):
    """One shape's data.  Gaussian codebook (scale 0.7) and vectors (scale 0.8); codes 7 (a NaN component) and 20 (an
    infinite one) are non-finite; two pairs of duplicated code vectors (duplicate_pairs).  From N = 33 on: vectors 2 and
    N - 3 sit exactly on the two duplicated codes, vector N // 2 holds a NaN and vector N // 3 an Inf.  Palettes (P = 4):
    row 0 everything (with the bits beyond K set as well), row 1 a random row (about 48 codes at K = 512, K / 3 otherwise),
    row 2 exactly 3 finite codes (plus a bit beyond K where the last word has room), row 3 empty; allowed_row random per
    vector, a few entries -1 and P, the planted vectors on row 0.  Output strides N + pad."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * N + 17 * D + K)
    E = torch.randn(K, D, generator=g) * 0.7
    z = torch.randn(N, D, generator=g) * 0.8
    dups = duplicate_pairs(K)
    for a, b in dups:
        E[b] = E[a]
    E[7, D // 2] = float("nan")
    E[20, 1] = float("-inf")
    planted = torch.zeros(N, dtype=torch.bool)
    on_dup = {}
    if N >= 33:
        on_dup = {2: dups[0], N - 3: dups[1]}
        for n, (a, _) in on_dup.items():
            z[n] = E[a]
        z[N // 2, D - 1] = float("nan")
        z[N // 3, 0] = float("inf")
        planted[[2, N - 3, N // 2, N // 3]] = True
    allowed = allowed_row = None
    if palettes:
        allowed = torch.zeros(4, K, dtype=torch.bool)
        allowed[0] = True
        allowed[1] = torch.rand(K, generator=g) < (48 / 512 if K >= 512 else 1 / 3)
        finite = [k for k in range(K) if k not in (7, 20)]
        pick = torch.randperm(len(finite), generator=g)[:3]
        allowed[2, [finite[int(i)] for i in pick]] = True
        allowed_row = torch.randint(0, 4, (N,), generator=g)
        if N >= 33:
            allowed_row[5], allowed_row[N - 7], allowed_row[17] = -1, 4, 4
            allowed_row[planted] = 0
    s_i, s_d = N + pad[0], N + pad[1]
    return SimpleNamespace(N=N, D=D, K=K, E=E, z=z, allowed=allowed, allowed_row=allowed_row, P=4 if palettes else 0,
                           ids_stride=s_i, dist_stride=s_d, dups=dups, on_dup=on_dup, planted=planted,
                           nan_vec=N // 2 if N >= 33 else None, inf_vec=N // 3 if N >= 33 else None)


def palette_words(case):
    """The word table int64 [P, W] (values 0 .. 2^32 - 1) of the case, rows 0 and 2 with bits beyond K set."""
    K, W = case.K, (case.K + 31) // 32
    bits = torch.zeros(case.P, W * 32, dtype=torch.int64)
    bits[:, :K] = case.allowed.long()
    bits[0, K:] = 1
    if W * 32 > K:
        bits[2, W * 32 - 1] = 1
    return (bits.reshape(case.P, W, 32) << torch.arange(32)).sum(-1)


def _once(case, name, make):
    """float64 work on a case is done once and kept on it (the cases are shared, never changed)"""
    if not hasattr(case, name):
        setattr(case, name, make())
    return getattr(case, name)


def rejected_share(case):
    """Share of the random (not planted) vectors that are not near-tie free, and the kept mask [N]."""
    def make():
        free = near_tie_free(case.z, case.E, case.allowed, case.allowed_row)
        random = ~case.planted
        return float((~free & random).sum()) / max(1, int(random.sum())), free & random
    return _once(case, "_rejected", make)


def empty_buffers(case, M):
    ids = torch.full((M * case.ids_stride + 11,), ID_POISON, dtype=torch.int64)
    dist = torch.full((M * case.dist_stride + 11,), DIST_POISON, dtype=torch.int32).view(torch.float32)
    return ids, dist


# ------------------------------------------------------------------------------------------ an fp32 model of the kernel
FAULTS = ["mask_ignored", "mask_row_next", "tie_high", "rank_dup", "merge_dropped_low", "merge_dropped_high", "padding_wins",
          "stride_ignored", "short_pad_zero"]


def model_f32(case, M, fault=None):
    """The kernel's arithmetic in fp32 on the padded codebook, written through the case's strides into poisoned flat
    buffers: (ids_buf, dist_buf).  `fault` plants one mistake: the mask ignored; the mask row of vector n + 1; ties to the
    higher index; rank 1 a copy of rank 0; the half-wave merge dropped (only the codes (r & 3) + 8 (r >> 2) of a tile, or
    only the + 4 half, are seen); padding codes k >= K winning (|e|^2 = 0 instead of +inf); the strides ignored; a short
    palette padded with code 0 instead of -1."""
    N, K, D = case.N, case.K, case.D
    Kp = (K + 31) // 32 * 32
    z, E = case.z, case.E
    cb = torch.zeros(Kp, D)
    cb[:K] = torch.where(torch.isfinite(E), E, torch.zeros_like(E))
    e2 = torch.full((Kp,), 0.0 if fault == "padding_wins" else float("inf"))
    e2[:K] = E.pow(2).sum(1)
    x2 = z.pow(2).sum(1, keepdim=True)
    with torch.no_grad():
        d = (x2 - 2.0 * (torch.where(torch.isfinite(z), z, torch.zeros_like(z)) @ cb.T)) + e2
    d[:, :K][:, ~torch.isfinite(E).all(1)] = float("inf")
    row = case.allowed_row
    if fault == "mask_row_next" and row is not None:
        row = torch.roll(row, -1)
    ok = torch.ones(N, Kp, dtype=torch.bool)
    if case.allowed is not None and fault != "mask_ignored":
        ok[:, :K] = allowed_matrix(N, K, case.allowed, row)
    k = torch.arange(Kp)
    if fault == "merge_dropped_low":
        ok &= ((k & 4) == 0)[None]
    if fault == "merge_dropped_high":
        ok &= ((k & 4) != 0)[None]
    d = torch.where(ok, d, torch.full_like(d, float("inf")))
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    if fault == "tie_high":
        order = torch.sort(d.flip(1), dim=1, stable=True)
        vals, idx = order.values, Kp - 1 - order.indices
    else:
        order = torch.sort(d, dim=1, stable=True)
        vals, idx = order.values, order.indices
    m = min(M, Kp)
    dist = torch.full((M, N), float("inf"))
    ids = torch.full((M, N), -1, dtype=torch.int64)
    dist[:m], ids[:m] = vals[:, :m].T, idx[:, :m].T
    missing = dist == float("inf")
    ids[missing] = 0 if fault == "short_pad_zero" else -1
    lost = ~(x2[:, 0] < float("inf"))
    ids[:, lost], dist[:, lost] = -1, float("nan")
    if fault == "rank_dup" and M >= 2:
        ids[1], dist[1] = ids[0], dist[0]
    ids_buf, dist_buf = empty_buffers(case, M)
    s_i, s_d = (N, N) if fault == "stride_ignored" else (case.ids_stride, case.dist_stride)
    for r in range(M):
        ids_buf[r * s_i:r * s_i + N] = ids[r]
        dist_buf[r * s_d:r * s_d + N] = dist[r]
    return ids_buf, dist_buf


# ------------------------------------------------------------------------------------------------------ the comparison
def unpack(buf, stride, N, M, poison, what):
    """[M, N] out of a flat buffer, and the assertion that nothing else of it was written"""
    b = buf.detach().cpu()
    raw = b.view(torch.int32) if b.dtype == torch.float32 else b
    inside = torch.zeros(b.numel(), dtype=torch.bool)
    for m in range(M):
        inside[m * stride:m * stride + N] = True
    assert bool((raw[~inside] == poison).all()), f"{what}: written outside [M][N] through the stride"
    return torch.stack([b[m * stride:m * stride + N] for m in range(M)])


def compare(ids_buf, dist_buf, case, M, what="", kept=None):
    """The kernel's flat outputs against the specification.  Returns (worst distance error / bound, number of certified
    near-tie swaps).  `kept` [N]: the vectors on which the ids must equal the spec's exactly (default: the near-tie-free
    random vectors of `rejected_share`)."""
    N, K = case.N, case.K
    ids = unpack(ids_buf, case.ids_stride, N, M, ID_POISON, what + " ids")
    dist = unpack(dist_buf, case.dist_stride, N, M, DIST_POISON, what + " dist")
    assert ids.dtype == torch.int64 and dist.dtype == torch.float32
    d64, S, x2, e2 = _once(case, "_d64", lambda: distances64(case.z, case.E))
    lost = torch.isnan(d64).any(1)
    may = allowed_matrix(N, K, case.allowed, case.allowed_row) & torch.isfinite(d64)
    count = may.sum(1)
    exists = (torch.arange(M)[:, None] < count[None]) & ~lost[None]
    # vectors without a distance; ranks without a code
    assert bool((ids[:, lost] == -1).all()) and bool(torch.isnan(dist[:, lost]).all()), f"{what}: a non-finite vector is not -1 / NaN"
    assert not bool(torch.isnan(dist[:, ~lost]).any()), f"{what}: NaN distance of a finite vector"
    assert torch.equal(ids >= 0, exists), f"{what}: the ranks that hold a code are not the first min(M, allowed) ones"
    assert bool((ids[~exists] == -1).all()), f"{what}: a missing rank is not id -1"
    gone = ~exists & ~lost[None]
    assert bool((dist[gone] == float("inf")).all()), f"{what}: a missing rank's distance is not +inf"
    # the codes returned: inside the codebook, allowed, finite, distinct
    assert bool((ids[exists] < K).all()), f"{what}: a padding code k >= K was returned"
    n_idx = torch.arange(N)[None].expand(M, N)
    assert bool(may[n_idx[exists], ids[exists]].all()), f"{what}: a code outside the palette (or a non-finite code) was returned"
    srt = torch.where(exists, ids, -1 - torch.arange(M)[:, None].expand(M, N)).sort(0).values
    assert bool((srt[1:] != srt[:-1]).all()), f"{what}: a code appears at two ranks"
    # the kernel's own order: (distance, id) ascending
    both = exists[:-1] & exists[1:]
    asc = (dist[:-1] < dist[1:]) | ((dist[:-1] == dist[1:]) & (ids[:-1] < ids[1:]))
    assert bool(asc[both].all()), f"{what}: ranks are not in (distance, index) order"
    # the distance bound
    safe = ids.clamp(min=0)
    want, mag = d64[n_idx, safe], S[n_idx, safe]
    err, lim = (dist.double() - want).abs()[exists], ((case.D + 3) * U * mag * (1 + 2.0 ** -20))[exists]
    ratio = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= lim).all()), f"{what}: worst distance error / bound = {ratio:.3f}"
    # the order against the specification
    spec_ids = _once(case, "_spec", lambda: topm_spec(case.z, case.E, GAP_RANKS, case.allowed, case.allowed_row))[0][:M]
    if kept is None:
        kept = rejected_share(case)[1]
    differ = ids != spec_ids
    assert not bool(differ[:, kept].any()), f"{what}: ids differ from the spec on near-tie-free vectors " \
                                            f"{differ[:, kept].any(0).nonzero().flatten().tolist()[:8]} (among the kept)"
    swaps = differ & exists
    if swaps.any():
        e2f = torch.where(torch.isfinite(e2), e2, torch.zeros_like(e2))
        sp = spec_ids.clamp(min=0)
        gap = (want - d64[n_idx, sp]).abs() / (x2[None] + e2f[sp])
        worst = float(gap[swaps].max())
        assert worst < CERTIFY, f"{what}: a swapped id is not a near-tie: normalised float64 gap {worst:.3e}"
    return ratio, int(swaps.sum())


def check_duplicates(ids_buf, dist_buf, case, M, what=""):
    """The vectors placed on a duplicated code: ranks 0 and 1 are the two duplicates, lower index first, at equal distance"""
    if M < 2:
        return
    ids = unpack(ids_buf, case.ids_stride, case.N, M, ID_POISON, what)
    dist = unpack(dist_buf, case.dist_stride, case.N, M, DIST_POISON, what)
    for n, (a, b) in case.on_dup.items():
        assert (int(ids[0, n]), int(ids[1, n])) == (a, b), f"{what}: vector {n} on codes {a} = {b} got {ids[:2, n].tolist()}"
        assert float(dist[0, n]) == float(dist[1, n]), f"{what}: duplicates at unequal distances"
