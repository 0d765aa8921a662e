"""Float64 specification of per-cell weighted mixtures of codebook rows (csrc/code_mix.hip, isi_embed_mix_f32), the test
data of its host and GPU tests, and the comparison both use.  CPU only.

For N cells, M sources (1 <= M <= 8), codebook E [K, D], ids [M, N] int64 and weights [M, N] fp32:

    mix[n, :] = sum over m ascending, of the terms with w[m, n] != 0, of  w[m, n] * E[id[m, n], :]

* A term whose weight compares equal to zero (+0.0 or -0.0) does not exist: its id is never looked at (-1, K, the priors'
  mask token, 2^40) and its codebook row may hold NaN.
* A term with a non-zero weight (NaN included) and an id outside [0, K) makes all D channels of that cell NaN, and only
  that cell's.
* The kernel's arithmetic for one lane is acc = -0.0f, then acc = fmaf(w, e, acc) for each existing term, m ascending: a
  cell whose only existing term has weight 1 is the codebook row bit for bit (-0.0 entries included), a cell with no
  existing term is -0.0, and a cell's bits depend on its own ids and weights alone.
* Error of the fp32 chain against the float64 sum: at most T * 2^-24 * sum_m |w_m e_m| * (1 + 2^-20), T the number of
  existing terms -- one rounding per fma, each bounded by 2^-24 of a partial sum that the absolute sum dominates.  (The
  data below keeps every product far above the subnormal range, where a rounding is absolute instead.)
"""
from types import SimpleNamespace

import torch

BIG = 2 ** 40
MASK_TOKEN = 1 << 15        # stands for the priors' mask token: any id >= K
OUT_POISON = 0x7FC12345     # a NaN no kernel produces: what the padding of an output buffer holds
NEG_ZERO_BITS = -2 ** 31


def mix_spec(ids, weights, E):
    """ids [M, N] int64, weights [M, N] fp32, E [K, D] -> (mix [N, D] float64 with NaN cells, mag [N, D] = sum |w e| over the
    existing terms, terms [N] = their number, bad [N] = a non-zero weight over an id outside [0, K))."""
    M, N = ids.shape
    K, D = E.shape
    Ed, wd = E.double(), weights.double()
    mix = torch.full((N, D), -0.0, dtype=torch.float64)
    mag = torch.zeros(N, D, dtype=torch.float64)
    terms = torch.zeros(N, dtype=torch.int64)
    bad = torch.zeros(N, dtype=torch.bool)
    for m in range(M):                                        # m ascending
        exists = weights[m] != 0                              # NaN != 0: a NaN weight is a term
        inside = (ids[m] >= 0) & (ids[m] < K)
        bad |= exists & ~inside
        use = exists & inside
        rows = Ed[torch.where(use, ids[m], torch.zeros_like(ids[m]))]          # an unused id is never an address
        prod = wd[m, :, None] * rows
        mix = torch.where(use[:, None], mix + prod, mix)
        mag = torch.where(use[:, None], mag + prod.abs(), mag)
        terms += exists
    mix[bad] = float("nan")
    return mix, mag, terms, bad


def bound(mag, terms):
    return terms[:, None].double() * 2.0 ** -24 * mag * (1 + 2.0 ** -20)


def fma32(a, b, c):
    """fp32 fmaf of fp32 tensors: the product of two fp32 numbers is exact in float64; the sum is rounded to float64 and
    then to fp32 (a double rounding differs from fmaf's single one in about one sum of 2^29)."""
    return (a.double() * b.double() + c.double()).float()


def model_f32(case, fault=None):
    """An fp32 model of the kernel, reading the case's flat buffers through its strides: [N, D] fp32.  `fault` plants one
    mistake: 'drop_term' (source 1, or source 0 when there is one source, is skipped), 'shifted_weights' (the weights of
    source m applied to source m + 1, the first source's to none: weight 1), 'zero_not_skipped', 'clamped_id', 'nan_leak'
    (a NaN cell also spoils the next cell), 'stride_ignored' (sources taken N elements apart), 'plus_zero' (acc = +0.0)."""
    N, M, K = case.N, case.M, case.K
    E = case.E
    s_i, s_w = (N, N) if fault == "stride_ignored" else (case.ids_stride, case.w_stride)
    acc = torch.full((N, case.D), 0.0 if fault == "plus_zero" else -0.0, dtype=torch.float32)
    bad = torch.zeros(N, dtype=torch.bool)
    for m in range(M):
        if fault == "drop_term" and m == min(1, M - 1):
            continue
        ids = case.ids_buf[m * s_i:m * s_i + N]
        if fault == "shifted_weights":
            w = case.w_buf[(m - 1) * s_w:(m - 1) * s_w + N] if m else torch.ones(N)
        else:
            w = case.w_buf[m * s_w:m * s_w + N]
        live = torch.ones(N, dtype=torch.bool) if fault == "zero_not_skipped" else w != 0
        inside = (ids >= 0) & (ids < K)
        if fault == "clamped_id":
            ids, inside = ids.clamp(0, K - 1), torch.ones(N, dtype=torch.bool)
        bad |= live & ~inside
        use = live & inside
        rows = E[torch.where(use, ids, torch.zeros_like(ids))]
        acc = torch.where(use[:, None], fma32(w[:, None], rows, acc), acc)
    acc[bad] = float("nan")
    if fault == "nan_leak":
        acc[torch.roll(bad, 1)] = float("nan")
    return acc


def bits(t):
    return t.contiguous().view(torch.int32)


def compare(got, case, what=""):
    """The comparison of the kernel's output [N, D] fp32 with the specification; returns the worst error / bound ratio.
    NaN exactly in the bad cells, all channels; -0.0 in a cell without a term; the codebook row's bits in a cell whose only
    existing term has weight 1; everywhere else the bound of the module's docstring."""
    ids, w, E = case.ids, case.weights, case.E
    mix, mag, terms, bad = mix_spec(ids, w, E)
    got = got.detach().cpu()
    assert got.shape == mix.shape and got.dtype == torch.float32, what
    nan = torch.isnan(got)
    assert torch.equal(nan.all(-1), bad) and torch.equal(nan.any(-1), bad), \
        f"{what}: NaN cells {nan.any(-1).nonzero().flatten().tolist()[:8]}, expected exactly {bad.nonzero().flatten().tolist()[:8]}"
    empty = (terms == 0) & ~bad
    assert bool((bits(got[empty]) == NEG_ZERO_BITS).all()), f"{what}: a cell without a term is not -0.0"
    exists = w != 0
    one = (terms == 1) & ~bad & ((exists & (w == 1)).sum(0) == 1)
    if one.any():
        src = (exists & (w == 1)).int().argmax(0)[one]
        rows = E[ids[src, one.nonzero().flatten()]]
        assert torch.equal(bits(got[one]), bits(rows)), f"{what}: a weight-1 cell is not the codebook row bit for bit"
    rest = ~bad & ~empty
    err, lim = (got.double() - mix).abs()[rest], bound(mag, terms)[rest]
    ratio = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0      # (a zero bound admits a zero error only)
    assert bool((err <= lim).all()), f"{what}: worst error / bound = {ratio:.3f}"
    return ratio


def make_case(N, M, D, K, seed=0, pad=(3, 5, 8)):
    """Test data for one shape: flat id / weight buffers with strides larger than N and independent of each other
    (ids_stride = N + pad[0], w_stride = N + pad[1]), ldo = D + pad[2].  The codebook holds -0.0 entries and, from K = 3 on,
    one row of NaN that no non-zero weight ever points at.  From N = 17 on the cells cycle through: general (signed weights
    that cancel in part), some weights +-0.0 over the ids -1, K, 2^40, the mask token and the NaN row, one-hot, all zero,
    an exact cancellation; and three cells carry an id outside [0, K) under a non-zero weight (one of them NaN).  Ids
    include 0 and K - 1."""
    g = torch.Generator().manual_seed(1000 * seed + 131 * N + 17 * M + D + K)
    E = torch.randn(K, D, generator=g)
    E[torch.rand(K, D, generator=g) < 0.05] = -0.0
    E[0, 0] = -0.0
    nan_row = 1 if K >= 3 else None
    valid = torch.tensor([k for k in range(K) if k != nan_row])
    if nan_row is not None:
        E[nan_row] = float("nan")
    ids = valid[torch.randint(0, len(valid), (M, N), generator=g)]
    w = torch.randn(M, N, generator=g)
    ids[0, 0], ids[-1, -1] = 0, K - 1
    hidden = [-1, K, BIG, MASK_TOKEN] + ([nan_row] if nan_row is not None else [])
    zero = lambda j: -0.0 if j & 1 else 0.0
    placed = [0]

    def hide(m, n):                                         # source m takes no part in cell n: its id is rubbish
        w[m, n], ids[m, n] = zero(placed[0] + placed[0] // len(hidden)), hidden[placed[0] % len(hidden)]
        placed[0] += 1

    bad_cells = {}
    if N >= 17:
        for n in range(1, N - 1):
            kind = n % 6
            if kind == 1:                                   # some sources absent
                for m in range(M):
                    if (n // 6 + m) % 2 == 0:
                        hide(m, n)
            elif kind == 2:                                 # one-hot
                hot = (n // 6) % M
                for m in range(M):
                    if m == hot:
                        w[m, n] = 1.0
                    else:
                        hide(m, n)
            elif kind == 3:                                 # no term at all
                for m in range(M):
                    hide(m, n)
            elif kind == 4 and M >= 2:                      # the first two terms cancel exactly
                ids[1, n], w[1, n] = ids[0, n], -w[0, n]
        last = max(n for n in range(1, N - 1) if n % 6 == 0)
        bad_cells = {5: (-1, 0.75), 6 * max(1, N // 12): (K, float("nan")), last: (BIG, -1.5)}      # general cells
        assert len(bad_cells) == 3
        for j, (n, (bad_id, bad_w)) in enumerate(bad_cells.items()):
            m = j % M
            ids[m, n], w[m, n] = bad_id, bad_w
    s_i, s_w, ldo = N + pad[0], N + pad[1], D + pad[2]
    ids_buf = torch.full((M * s_i,), BIG + 7, dtype=torch.int64)
    w_buf = torch.full((M * s_w,), 7.0)
    for m in range(M):
        ids_buf[m * s_i:m * s_i + N] = ids[m]
        w_buf[m * s_w:m * s_w + N] = w[m]
    return SimpleNamespace(N=N, M=M, D=D, K=K, E=E, ids=ids, weights=w, ids_buf=ids_buf, ids_stride=s_i, w_buf=w_buf,
                           w_stride=s_w, ldo=ldo, nan_row=nan_row, bad_cells=sorted(bad_cells))
