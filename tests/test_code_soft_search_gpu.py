"""GPU tests of the code-database search by encoder vectors (csrc/code_search.hip, csrc/code_shift_search.hip; DESIGN.md
section 6c.2) through the C-ABI and through `CodeIndex`, against the float64 / int64 specification
tests/code_soft_search_spec.py: the rows builder's bound and its bit-identity with the code distance table; the aligned and
the shifted rows searches on every route of the hard searches' tests -- exact on integer rows, inside the derived bound and
bitwise the fp32 emulation on float rows, NaN and inf under zero weights, and bit for bit the hard searches on gathered
table rows (contracts 1 to 4); determinism and item-locality; sentinel margins around every buffer the kernels write or
stream; and `encode_vectors`, `search_soft`, `search_shifted_soft` and the `inpainting` entry points on a fixture VQ-VAE."""
import functools

import numpy as np
import pytest
import torch

import code_search_spec as S
import code_shift_search_spec as SH
import code_soft_search_spec as R
from test_code_shift_search_gpu import SHAPES as SHIFT_SHAPES

pytestmark = pytest.mark.gpu

MARGIN = 64                 # sentinel elements on each side of a guarded buffer (keeps 16-byte alignment of the payload)
SENTINEL_F = -12345.0
SENTINEL_U = 0x5A5A

ROUTES = [(1, 1, 2, 1), (1000, 1024, 512, 1), (257, 4096, 512, 2), (1031, 77, 300, 3), (64, 1000, 1024, 1)]
CHUNKS = [(300, 264, 600, 2), (200, 72, 1500, 1), (100, 40, 3000, 1), (50, 16, 4100, 1)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Guarded:
    """A device buffer with sentinel-filled margins; `shift` elements move the payload off its natural alignment."""

    def __init__(self, shape, dtype, fill, dev, shift=0):
        self.n = int(np.prod(shape))
        self.fill = fill
        self.lo = MARGIN + shift
        self.raw = torch.full((self.n + 2 * MARGIN + shift,), fill, dtype=dtype, device=dev)
        self.view = self.raw[self.lo:self.lo + self.n].view(*shape)

    def intact(self):
        return bool((self.raw[:self.lo] == self.fill).all()) and bool((self.raw[self.lo + self.n:] == self.fill).all())


def _u16(array, dev, shift=0):
    g = _Guarded(array.shape, torch.int16, SENTINEL_U, dev, shift)
    g.view.copy_(torch.from_numpy(array.astype(np.uint16).view(np.int16)))
    return g


def _f32(array, dev, shift=0):
    g = _Guarded(array.shape, torch.float32, SENTINEL_F, dev, shift)
    g.view.copy_(torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)))
    return g


# ---------------------------------------------------------------------------------------------------- the rows builder
def _build_rows(lib, dev, z, E, pad=0):
    """isi_code_query_rows_f32 on guarded buffers -> rows [cells, K] (numpy).  pad > 0: the vectors lie at a stride of
    D + pad floats, with NaN between them -- nothing outside a vector may be read."""
    cells, D = z.shape
    K = E.shape[0]
    wide = np.full((cells, D + pad), np.nan, np.float32)
    wide[:, :D] = z
    g_z, g_E = _f32(wide, dev), _f32(E, dev)
    g_rows = _Guarded((cells, K), torch.float32, SENTINEL_F, dev)
    rc = lib.isi_code_query_rows_f32(g_z.view.data_ptr(), D + pad, g_E.view.data_ptr(), g_rows.view.data_ptr(), cells, K, D, None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert g_rows.intact() and g_z.intact() and g_E.intact()
    assert np.array_equal(_bits(g_E.view.cpu().numpy()), _bits(E))                     # read, never written
    return g_rows.view.cpu().numpy()


@pytest.mark.parametrize("cells,K,D", [(1, 2, 1), (77, 300, 64), (4096, 512, 64), (1000, 1024, 32), (40, 7, 3)])
def test_rows_bound_and_table_rows_bit_for_bit(cells, K, D):
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    rng = np.random.default_rng(cells + K + D)
    E = rng.standard_normal((K, D)).astype(np.float32)
    z = rng.standard_normal((cells, D)).astype(np.float32)
    picks = rng.integers(0, K, cells)
    copied = np.arange(cells) % 2 == 0                                # every other vector IS a codebook row
    z[copied] = E[picks[copied]]
    rows = _build_rows(lib, dev, z, E)
    r64 = R.rows64(z, E)
    err, bound = np.abs(rows.astype(np.float64) - r64), R.rows_bound(r64, D)
    print(f"rows cells={cells} K={K} D={D}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(_bits(rows), _bits(_build_rows(lib, dev, z, E, pad=5)))      # z_stride == D + 5: the same bits
    # contract 1: bit for bit the table kernel's rows
    g_T = _Guarded((K, K), torch.float32, SENTINEL_F, dev)
    d_E = torch.from_numpy(E).to(dev)
    assert lib.isi_code_distance_table_f32(d_E.data_ptr(), g_T.view.data_ptr(), K, D, None) == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    T = g_T.view.cpu().numpy()
    assert np.array_equal(_bits(rows[copied]), _bits(T[picks[copied]]))
    assert (rows[copied, picks[copied]] == 0).all()
    # a NaN vector poisons its own row and no other; an infinite component gives an infinite row
    bad = z.copy()
    bad[cells // 2, D - 1] = np.nan
    poisoned = _build_rows(lib, dev, bad, E)
    assert np.isnan(poisoned[cells // 2]).all()
    keep = np.arange(cells) != cells // 2
    assert np.array_equal(_bits(poisoned[keep]), _bits(rows[keep]))
    bad[cells // 2, D - 1] = np.inf
    assert np.isposinf(_build_rows(lib, dev, bad, E)[cells // 2]).all()


# ------------------------------------------------------------------------------------------------- the aligned search
def _rows_search(lib, dev, codes, rows, w, allowed=None, prefill=None, shift=0, rows_shift=0):
    """One isi_code_search_rows_f32 call on guarded buffers -> dist [Q, N] float32 (numpy); the margins are asserted."""
    N, C = codes.shape
    Q, K = rows.shape[0], rows.shape[2]
    g_codes = _u16(codes, dev, shift)
    g_rows = _f32(rows, dev, rows_shift)
    d_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
    d_allowed = None if allowed is None else torch.from_numpy(np.ascontiguousarray(allowed, dtype=np.uint8)).to(dev)
    g_dist = _Guarded((Q, N), torch.float32, SENTINEL_F, dev)
    if prefill is not None:
        g_dist.view.copy_(torch.from_numpy(np.ascontiguousarray(prefill, dtype=np.float32)))
    need = lib.isi_code_search_workspace_bytes(N, C, K, Q)
    g_ws = _Guarded((need // 4,), torch.float32, SENTINEL_F, dev)
    rc = lib.isi_code_search_rows_f32(g_codes.view.data_ptr(), g_rows.view.data_ptr(), None if d_w is None else d_w.data_ptr(),
                                      None if d_allowed is None else d_allowed.data_ptr(), g_dist.view.data_ptr(), N, C, K, Q,
                                      int(prefill is not None), g_ws.view.data_ptr(), need, None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert g_dist.intact() and g_ws.intact() and g_codes.intact() and g_rows.intact()
    assert np.array_equal(g_codes.view.cpu().numpy().view(np.uint16), codes)          # streamed, never written
    return g_dist.view.cpu().numpy()


def _hard_search(lib, dev, codes, query, w, table):
    N, C = codes.shape
    Q, K = query.shape[0], table.shape[0]
    d_codes, d_query = (torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev) for a in (codes, query))
    d_w, d_table = torch.from_numpy(w).to(dev), torch.from_numpy(table).to(dev)
    dist = torch.empty(Q, N, dtype=torch.float32, device=dev)
    need = lib.isi_code_search_workspace_bytes(N, C, K, Q)
    ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=dev)
    assert lib.isi_code_search_f32(d_codes.data_ptr(), d_query.data_ptr(), d_w.data_ptr(), d_table.data_ptr(), None,
                                   dist.data_ptr(), N, C, K, Q, 0, ws.data_ptr(), need, None) == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    return dist.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(N, C, K, Q, seed, integer):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, K, (N, C)).astype(np.uint16)
    codes[N - 1, C - 1] = K - 1
    codes[0, 0] = K - 1
    if integer:
        rows = rng.integers(0, 256, (Q, C, K), dtype=np.uint8).astype(np.float32)     # independent per cell: a swap shows
        w = (rng.random((Q, C)) < 0.7).astype(np.float32)
        w[0, 0] = 1.0
    else:
        rows = (rng.standard_normal((Q, C, K), dtype=np.float32) ** 2 * 16).astype(np.float32)
        w = (2.0 * rng.random((Q, C))).astype(np.float32)
    return codes, rows, w                                             # shared among the tests: nobody changes them


def _exact_checks(lib, dev, N, C, K, Q, seed):
    codes, rows, w = _inputs(N, C, K, Q, seed, True)
    want = R.search_int(codes, rows, w)
    assert want.max() + 1000 < 2 ** 24
    allowed = (np.arange(N) % 3 != 1).astype(np.uint8)
    got = _rows_search(lib, dev, codes, rows, w, allowed=allowed)
    assert np.array_equal(got.astype(np.float64), R.apply_allowed(want, allowed))
    prefill = np.random.default_rng(N).integers(0, 1000, (Q, N)).astype(np.float32)
    acc = _rows_search(lib, dev, codes, rows, w, prefill=prefill)
    assert np.array_equal(acc.astype(np.int64), want + prefill.astype(np.int64))
    # the rows base moved by one float: the scalar stage, the same bits; the codes base moved: the scalar code route
    assert np.array_equal(_bits(_rows_search(lib, dev, codes, rows, w, allowed=allowed, rows_shift=1)), _bits(got))
    assert np.array_equal(_bits(_rows_search(lib, dev, codes, rows, w, allowed=allowed, shift=1)), _bits(got))
    # null weights: 1 on every cell
    none = _rows_search(lib, dev, codes, rows, None)
    assert np.array_equal(none.astype(np.int64), R.search_int(codes, rows, None))
    # NaN and inf rows under zero weights change nothing
    dead = np.argwhere(w == 0)
    if len(dead):
        poisoned = rows.copy()
        poisoned[dead[::2, 0], dead[::2, 1], :] = np.nan
        poisoned[dead[1::2, 0], dead[1::2, 1], :] = np.inf
        for rows_shift in (0, 1):
            again = _rows_search(lib, dev, codes, poisoned, w, allowed=allowed, rows_shift=rows_shift)
            assert np.array_equal(_bits(again), _bits(got))


@pytest.mark.parametrize("N,C,K,Q", ROUTES)
def test_exact_rows_search_on_integer_rows(N, C, K, Q):
    """Integer rows in [0, 255], 0/1 weights, sums below 2^24: bitwise the int64 specification, with `allowed`, accumulated
    onto a prefill, from a rows base one float off its alignment, with null weights, and with NaN / inf rows under the
    zero weights."""
    from interactive_spectrogram_inpainting import _hip
    _exact_checks(_hip.lib(), _dev(), N, C, K, Q, 100 + N)


@pytest.mark.parametrize("N,C,K,Q", CHUNKS)
def test_exact_rows_search_on_every_chunk_size(N, C, K, Q):
    """The chunk of staged cells shrinks with K (24, 8, 5 and 3 cells) and C = 264 leaves a second run of 8 cells."""
    from interactive_spectrogram_inpainting import _hip
    _exact_checks(_hip.lib(), _dev(), N, C, K, Q, 300 + N)


@pytest.mark.parametrize("N,C,K,Q", ROUTES + CHUNKS)
def test_float_rows_search_inside_the_derived_bound(N, C, K, Q):
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    codes, rows, w = _inputs(N, C, K, Q, 200 + N, False)
    want, mag = R.search64(codes, rows, w)
    got = _rows_search(lib, dev, codes, rows, w)
    err, bound = np.abs(got.astype(np.float64) - want), R.search_bound(mag, C)
    print(f"rows search N={N} C={C} K={K} Q={Q}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all()
    assert np.array_equal(_bits(got), _bits(R.emulate_f32(codes, rows, w)))            # the documented summation order
    assert np.array_equal(_bits(_rows_search(lib, dev, codes, rows, w, rows_shift=1)), _bits(got))


@pytest.mark.parametrize("N,C,K,Q", ROUTES + CHUNKS)
def test_gathered_table_rows_equal_the_hard_search_bit_for_bit(N, C, K, Q):
    """Contract 2: rows[j][c] = T[query[j][c]], mask-token cells under weight 0 in both calls."""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    rng = np.random.default_rng(500 + N)
    codes = rng.integers(0, K, (N, C)).astype(np.uint16)
    query = rng.integers(0, K, (Q, C)).astype(np.uint16)
    if C > 1:
        query[rng.random((Q, C)) < 0.15] = K
    table = S.table64(rng.standard_normal((K, 16)).astype(np.float32)).astype(np.float32)
    w = R.mask_token_weights(query, (2.0 * rng.random((Q, C))).astype(np.float32), K)
    hard = _hard_search(lib, dev, codes, query, w, table)
    soft = _rows_search(lib, dev, codes, R.gather_rows(table, query), w)
    assert np.array_equal(_bits(soft), _bits(hard))


def test_deterministic_and_item_local():
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    N, C, K, Q = 1000, 1024, 512, 3
    codes, rows, w = _inputs(N, C, K, Q, 7, False)
    codes = codes.copy()
    codes[500] = codes[20]                                            # the same sound stored twice
    full = _rows_search(lib, dev, codes, rows, w)
    assert np.array_equal(_bits(full), _bits(_rows_search(lib, dev, codes, rows, w)))
    assert np.array_equal(_bits(full[:, 500]), _bits(full[:, 20]))
    alone = _rows_search(lib, dev, codes[100:200].copy(), rows, w)
    assert np.array_equal(_bits(alone), _bits(full[:, 100:200]))
    for j in range(Q):
        one = _rows_search(lib, dev, codes, rows[j:j + 1], w[j:j + 1])
        assert np.array_equal(_bits(one[0]), _bits(full[j]))
    assert np.array_equal(_bits(full), _bits(_rows_search(lib, dev, codes, rows, w, shift=1)))


# ------------------------------------------------------------------------------------------------- the shifted search
def _shift_rows_search(lib, dev, codes, rows, w, W, shift0, step, count, prefill=None, shift=0, rows_shift=0):
    """One isi_code_shift_search_rows_f32 call on guarded buffers -> dist [Q, S, N] float32 (numpy)."""
    N, F, T = codes.shape
    Q, K = rows.shape[0], rows.shape[2]
    g_codes = _u16(codes, dev, shift)
    g_rows = _f32(rows, dev, rows_shift)
    d_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
    g_dist = _Guarded((Q, count, N), torch.float32, SENTINEL_F, dev)
    if prefill is not None:
        g_dist.view.copy_(torch.from_numpy(np.ascontiguousarray(prefill, dtype=np.float32)))
    need = lib.isi_code_shift_search_workspace_bytes(N, F, T, W, count, K, Q)
    g_ws = _Guarded((need // 4,), torch.float32, SENTINEL_F, dev)
    rc = lib.isi_code_shift_search_rows_f32(g_codes.view.data_ptr(), g_rows.view.data_ptr(),
                                            None if d_w is None else d_w.data_ptr(), g_dist.view.data_ptr(), N, F, T, W, shift0,
                                            step, count, K, Q, int(prefill is not None), g_ws.view.data_ptr(), need, None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert g_dist.intact() and g_ws.intact() and g_codes.intact() and g_rows.intact()
    assert np.array_equal(g_codes.view.cpu().numpy().view(np.uint16), codes)
    return g_dist.view.cpu().numpy()


def _hard_shift_search(lib, dev, codes, query, w, table, shift0, step, count):
    N, F, T = codes.shape
    Q, W, K = query.shape[0], query.shape[2], table.shape[0]
    d_codes, d_query = (torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev) for a in (codes, query))
    d_w, d_table = torch.from_numpy(w).to(dev), torch.from_numpy(table).to(dev)
    dist = torch.empty(Q, count, N, dtype=torch.float32, device=dev)
    need = lib.isi_code_shift_search_workspace_bytes(N, F, T, W, count, K, Q)
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    rc = lib.isi_code_shift_search_f32(d_codes.data_ptr(), d_query.data_ptr(), d_w.data_ptr(), d_table.data_ptr(),
                                       dist.data_ptr(), N, F, T, W, shift0, step, count, K, Q, 0, ws.data_ptr(), need, None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    return dist.cpu().numpy()


@pytest.mark.parametrize("shape", SHIFT_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_exact_shifted_rows_search_and_the_hard_search_bit_for_bit(shape):
    """Every shape family of the hard shifted search's tests (one run and several, step > 1, shift0 > 0, both routes):
    integer window rows are bitwise the int64 specification -- also from misaligned codes and rows, accumulated onto a
    prefill, with null weights and with NaN rows under zero weights -- and gathered table rows give
    isi_code_shift_search_f32's bits (contract 3)."""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    N, F, T, W, shift0, step, count, K, Q = shape
    rng = np.random.default_rng(700 + N)
    codes = rng.integers(0, K, (N, F, T)).astype(np.uint16)
    codes[N - 1, F - 1, T - 1] = codes[0, 0, 0] = K - 1
    rows = rng.integers(0, 256, (Q, F * W, K), dtype=np.uint8).astype(np.float32)
    w = (rng.random((Q, F, W)) < 0.7).astype(np.float32)
    w[0, 0, 0] = 1.0
    want = R.shift_search_int(codes, rows, w, W, shift0, step, count)
    assert want.max() + 1000 < 2 ** 24 and want.shape == (Q, count, N)
    got = _shift_rows_search(lib, dev, codes, rows, w, W, shift0, step, count)
    assert np.array_equal(got.astype(np.int64), want)
    off = _shift_rows_search(lib, dev, codes, rows, w, W, shift0, step, count, shift=1, rows_shift=1)
    assert np.array_equal(_bits(off), _bits(got))
    prefill = np.random.default_rng(N).integers(0, 1000, (Q, count, N)).astype(np.float32)
    acc = _shift_rows_search(lib, dev, codes, rows, w, W, shift0, step, count, prefill=prefill)
    assert np.array_equal(acc.astype(np.int64), want + prefill.astype(np.int64))
    none = _shift_rows_search(lib, dev, codes, rows, None, W, shift0, step, count)
    assert np.array_equal(none.astype(np.int64), R.shift_search_int(codes, rows, None, W, shift0, step, count))
    dead = np.argwhere(w.reshape(Q, -1) == 0)
    if len(dead):
        poisoned = rows.copy()
        poisoned[dead[:, 0], dead[:, 1], :] = np.nan
        assert np.array_equal(_bits(_shift_rows_search(lib, dev, codes, poisoned, w, W, shift0, step, count)), _bits(got))
    # contract 3, on a float table with mask-token cells
    query = rng.integers(0, K, (Q, F, W)).astype(np.uint16)
    if F * W > 1:
        query[rng.random((Q, F, W)) < 0.15] = K
    table = S.table64(rng.standard_normal((K, 16)).astype(np.float32)).astype(np.float32)
    wf = R.mask_token_weights(query, (2.0 * rng.random((Q, F, W))).astype(np.float32), K)
    hard = _hard_shift_search(lib, dev, codes, query, wf, table, shift0, step, count)
    gathered = R.gather_rows(table, query.reshape(Q, -1))
    soft = _shift_rows_search(lib, dev, codes, gathered, wf, W, shift0, step, count)
    assert np.array_equal(_bits(soft), _bits(hard))
    ref, mag = R.shift_search64(codes, gathered, wf, W, shift0, step, count)
    err, bound = np.abs(soft.astype(np.float64) - ref), R.shift_bound(mag, F, W)
    print(f"shifted rows search {shape}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("N,F,T,K,Q", [(100, 3, 40, 600, 1), (300, 16, 64, 512, 2), (70, 7, 11, 300, 2)])
def test_full_width_equals_the_aligned_rows_search_bit_for_bit(N, F, T, K, Q):
    """Contract 4: W == T, S == 1, shift0 == 0 (one run, four runs, an odd pitch)."""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    codes, rows, w = _inputs(N, F * T, K, Q, 400 + N, False)
    shifted = _shift_rows_search(lib, dev, codes.reshape(N, F, T), rows, w.reshape(Q, F, T), T, 0, 1, 1)
    assert np.array_equal(_bits(shifted[:, 0]), _bits(_rows_search(lib, dev, codes, rows, w)))
    assert np.array_equal(_bits(shifted[:, 0]), _bits(R.emulate_f32(codes, rows, w)))


# ------------------------------------------------------------------------------------------------------- end to end
class _Enc:                                      # stands in for sklearn's LabelEncoder
    def __init__(self, classes):
        self.classes = list(classes)

    def transform(self, values):
        return np.array([self.classes.index(v) for v in values])

    def inverse_transform(self, indexes):
        return np.array([self.classes[int(i)] for i in indexes], dtype=object)


def test_code_index_soft_end_to_end():
    import inpainting
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.datasets.code_index import CodeIndex
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    dev, K = _dev(), 32
    torch.manual_seed(11)
    vq = VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
               num_embeddings=K, resolution_factors={"bottom": 4, "top": 2}).to(dev).eval()
    g = torch.Generator().manual_seed(12)
    # an "upload": its vectors, and the codes they snap to
    spectrogram = torch.randn(1, 2, 64, 32, generator=g).to(dev)
    z_t, z_b, id_t, id_b = vq.encode_vectors(spectrogram)
    codes_t, _, codes_b, _ = vq.encode_topm(spectrogram, 1)
    assert z_t.shape == (1, 8, 4, 16) and z_b.shape == (1, 16, 8, 16) and z_t.dtype == torch.float32
    assert id_t.dtype == torch.int64 and torch.equal(id_t, codes_t[0]) and torch.equal(id_b, codes_b[0])
    for z, ids, quantizer in ((z_t, id_t, vq.quantize_t), (z_b, id_b, vq.quantize_b)):
        rows = quantizer.distance_rows(z)
        assert rows.shape == ids.shape + (K,)
        E = quantizer.embed.detach().t().cpu().numpy()
        r64 = R.rows64(z.reshape(-1, 16).cpu().numpy(), E)
        assert (np.abs(rows.reshape(-1, K).cpu().numpy() - r64) <= R.rows_bound(r64, 16)).all()
        near = np.take_along_axis(r64, ids.reshape(-1, 1).cpu().numpy(), 1)[:, 0]
        assert (near <= r64.min(1) * (1 + 1e-5)).all()                 # the snapped code is the row's minimum
    N, COPY, SNAP = 500, 124, 77
    top, bottom = torch.randint(0, K, (N, 8, 4), generator=g), torch.randint(0, K, (N, 16, 8), generator=g)
    top[300], bottom[300] = top[40], bottom[40]
    top[COPY], bottom[COPY] = top[40], bottom[40]
    changed = [(0, 0), (2, 1), (3, 3), (5, 2), (7, 0)]
    for f, t in changed:
        top[COPY, f, t] = (top[40, f, t] + 1 + 3 * f) % K
    top[SNAP], bottom[SNAP] = id_t[0].cpu(), id_b[0].cpu()            # the upload's own codes are in the database
    encoders = {"pitch": _Enc(range(24, 85)), "instrument_family_str": _Enc([f"fam{i}" for i in range(11)])}
    attrs = {"pitch": torch.arange(N) % 61, "instrument_family_str": torch.arange(N) % 11}
    index = CodeIndex.from_arrays(top, bottom, attrs, vq, dev, encoders)
    q_top, q_bottom = top[40].to(dev), bottom[40].to(dev)
    v_top, v_bottom = vq.quantize_t.embed_code(q_top.unsqueeze(0)), vq.quantize_b.embed_code(q_bottom.unsqueeze(0))
    assert v_top.shape == (1, 8, 4, 16)
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))                     # noqa: E731  indices and bits
    # vectors that ARE codebook rows: the hard search's indices and, bit for bit, its distances -- over the whole ranking
    hard = index.search(q_top, q_bottom, k=N)
    soft = index.search_soft(top_vectors=v_top[0], bottom_vectors=v_bottom[0], k=N)
    assert soft[0].dtype == torch.int64 and soft[1].dtype == torch.float32 and soft[0].shape == (N,)
    assert same(soft, hard) and soft[0][:3].tolist() == [40, 300, COPY] and soft[1][:2].tolist() == [0.0, 0.0]
    # a vectors layer beside a codes layer, either way round; rows handed over ready; one layer alone; a layer weight
    assert same(index.search_soft(bottom_code=q_bottom, top_vectors=v_top, k=N), hard)
    assert same(index.search_soft(q_top, bottom_vectors=v_bottom, k=N), hard)
    assert same(index.search_soft(q_top, q_bottom, k=N), hard)
    ready = vq.quantize_t.distance_rows(v_top)
    assert same(index.search_soft(top_rows=ready, bottom_code=q_bottom, k=N), hard)
    assert same(index.search_soft(top_vectors=v_top, k=5), index.search(q_top, k=5))
    assert same(index.search_soft(top_vectors=v_top, bottom_vectors=v_bottom, layer_weights=(1.0, 0.5), k=N),
                index.search(q_top, q_bottom, layer_weights=(1.0, 0.5), k=N))
    # masks (True = weight 0; NaN under the mask counts nothing) and constraints
    hole = torch.zeros(8, 4, dtype=torch.bool, device=dev)
    for f, t in changed:
        hole[f, t] = True
    holed = v_top.clone()
    holed[0][hole] = float("nan")
    found = index.search_soft(top_vectors=holed, bottom_vectors=v_bottom, mask_top=hole, k=3)
    assert found[0].tolist() == [40, COPY, 300] and found[1].tolist() == [0.0, 0.0, 0.0]
    assert same(found, index.search(q_top, q_bottom, mask_top=hole, k=3))
    found = index.search_soft(top_vectors=v_top, bottom_vectors=v_bottom, k=2, attribute_constraints={"instrument_family_str": "fam3"})
    assert found[0].tolist() == [300, COPY]
    assert index.search_soft(top_vectors=v_top, bottom_vectors=v_bottom, k=2, exclude=[40])[0].tolist() == [300, COPY]
    with pytest.raises(LookupError):
        index.search_soft(top_vectors=v_top, attribute_constraints={"pitch": 1000})
    # the batched form, in groups of queries: the grouping changes no bit
    from interactive_spectrogram_inpainting.utils.datasets import code_index
    batch_t = vq.quantize_t.embed_code(top[[40, 7, 9]].to(dev))
    batch_b = vq.quantize_b.embed_code(bottom[[40, 7, 9]].to(dev))
    both = index.search_soft(top_vectors=batch_t, bottom_vectors=batch_b, k=2)
    assert both[0].shape == (3, 2) and both[0][:, 0].tolist() == [40, 7, 9] and both[1][:, 0].tolist() == [0.0, 0.0, 0.0]
    budget = code_index.ROWS_BUDGET_BYTES
    try:
        code_index.ROWS_BUDGET_BYTES = 16 * 8 * K * 4                  # one query's bottom rows at a time
        assert same(index.search_soft(top_vectors=batch_t, bottom_vectors=batch_b, k=2), both)
    finally:
        code_index.ROWS_BUDGET_BYTES = budget
    # the upload itself: the item that holds its snapped codes is the nearest one, at the sum of the rows' minima
    found = inpainting.similar_sounds_to_spectrogram(index, vq, spectrogram, k=3)
    snapped = inpainting.similar_sounds(index, id_t, id_b, k=3)
    (f_top, f_bottom), f_attrs, f_dist = found[0]
    assert torch.equal(f_top.cpu(), top[SNAP:SNAP + 1]) and torch.equal(f_bottom.cpu(), bottom[SNAP:SNAP + 1])
    assert torch.equal(snapped[0][0][0].cpu(), top[SNAP:SNAP + 1]) and snapped[0][2] == 0.0 and f_attrs == snapped[0][1]
    lower = sum(float(R.rows64(z.reshape(-1, 16).cpu().numpy(), q.embed.detach().t().cpu().numpy()).min(1).sum())
                for z, q in ((z_t, vq.quantize_t), (z_b, vq.quantize_b)))
    assert f_dist > 0 and abs(f_dist - lower) <= 1e-4 * lower and found[1][2] > f_dist
    direct = index.search_soft(top_vectors=z_t, bottom_vectors=z_b, k=3)
    assert [f[2] for f in found] == direct[1].tolist()
    masked = inpainting.similar_sounds_to_spectrogram(index, vq, spectrogram, mask=hole.unsqueeze(0), layer="top", k=2)
    assert torch.equal(masked[0][0][0].cpu(), top[SNAP:SNAP + 1]) and 0 < masked[0][2] < f_dist
    # a morph at one-hot weights is `similar_sounds` on the codes it selects, bit for bit
    two_t = torch.stack([q_top.unsqueeze(0), top[7:8].to(dev)])
    two_b = torch.stack([q_bottom.unsqueeze(0), bottom[7:8].to(dev)])
    one_hot = lambda c: torch.stack([torch.ones_like(c[0], dtype=torch.float32), torch.zeros_like(c[0], dtype=torch.float32)])  # noqa: E731
    mixture = inpainting.similar_to_mixture(index, vq, two_t, one_hot(two_t), two_b, one_hot(two_b), k=4)
    plain = inpainting.similar_sounds(index, q_top.unsqueeze(0), q_bottom.unsqueeze(0), k=4)
    assert [m[2] for m in mixture] == [p[2] for p in plain] and [m[1] for m in mixture] == [p[1] for p in plain]
    assert all(torch.equal(m[0][0], p[0][0]) and torch.equal(m[0][1], p[0][1]) for m, p in zip(mixture, plain))
    half = torch.full_like(one_hot(two_t), 0.5)
    blend = inpainting.similar_to_mixture(index, vq, two_t, half, two_b, torch.full_like(one_hot(two_b), 0.5), k=N)
    assert {int(b[1]["pitch"]) for b in blend[:4]} >= {24 + 40, 24 + 7} and blend[0][2] > 0    # both parents lead a half-way blend
    # the shifted form: windows of vectors that are codebook rows give `search_shifted`'s results bit for bit
    hard = index.search_shifted(q_top[:, 1:3], q_bottom[:, 2:6], k=N)
    soft = index.search_shifted_soft(top_vectors=v_top[:, :, 1:3], bottom_vectors=v_bottom[:, :, 2:6], k=N)
    assert same(soft, hard) and int(soft[0][0]) == 40 and int(soft[1][0]) == 1
    assert same(index.search_shifted_soft(q_top[:, 1:3], bottom_vectors=v_bottom[:, :, 2:6], k=N), hard)
    assert same(index.search_shifted_soft(top_vectors=v_top[:, :, 1:3], k=N, shift_range=(1, 3)),
                index.search_shifted(q_top[:, 1:3], k=N, shift_range=(1, 3)))
    assert torch.equal(index.distances_shifted_soft(top_vectors=v_top[:, :, 1:3], bottom_vectors=v_bottom[:, :, 2:6]),
                       index.distances_shifted(q_top[:, 1:3], q_bottom[:, 2:6]))
    fragments = inpainting.similar_fragments_to_spectrogram(index, vq, spectrogram, 1, 2, k=2)
    assert torch.equal(fragments[0][0][0].cpu(), top[SNAP:SNAP + 1]) and fragments[0][3] == 1 and fragments[0][2] > 0
    # no CPU path
    with pytest.raises(_hip.HipLibraryError):
        index.search_soft(top_vectors=v_top.cpu(), bottom_vectors=v_bottom.cpu())
    with pytest.raises(_hip.HipLibraryError):
        index.search_shifted_soft(top_vectors=v_top[:, :, 1:3].cpu())
    with pytest.raises(ValueError):
        index.search_soft(top_vectors=v_top[:, :, :3])
