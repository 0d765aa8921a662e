"""GPU tests of the time-warped code search (csrc/code_warp_search.hip) through the C-ABI and through
`CodeIndex`, against the specification tests/code_warp_search_spec.py on the geometries and inputs of
tests/test_code_warp_search_host.py: per geometry exact equality on integer rows, the fp32 emulation bit for bit on float
rows and the derived bound; bit-identity under permuting the database, changing N and Q and misaligning the codes; the
closed band against the shifted search; monotonicity under nested bands; `allowed`; the path kernel; a planted warp; the
refusals; sentinel margins around every buffer the kernels write or stream; and `search_warped`, `warp_paths`,
`similar_sounds_warped` and `paste_warped` on a small index."""
import numpy as np
import pytest
import torch

import code_shift_search_spec as SH
import code_soft_search_spec as R
import code_warp_search_spec as WS
from test_code_warp_search_host import IDS, check_cabi_refusals, geometry, parts_of, reference, reference64

pytestmark = pytest.mark.gpu

MARGIN = 64                 # sentinel elements on each side of a guarded buffer (keeps 16-byte alignment of the payload)
SENTINEL_F = -12345.0
SENTINEL_U = 0x5A5A
SENTINEL_I = -777


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
    g.view.copy_(torch.from_numpy(np.ascontiguousarray(array).astype(np.uint16).view(np.int16)))
    return g


def _f32(array, dev, shift=0):
    g = _Guarded(array.shape, torch.float32, SENTINEL_F, dev, shift)
    g.view.copy_(torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32)))
    return g


class _Device:
    """The parts of one search on guarded device buffers, and the isi_warp_part array that points into them."""

    def __init__(self, parts, dev, shift=0, rows_shift=0):
        from interactive_spectrogram_inpainting import _hip
        self.parts = parts
        self.codes = [_u16(p.codes, dev, shift) for p in parts]
        self.rows = [_f32(p.rows, dev, rows_shift) for p in parts]
        self.weights = [None if p.weights is None else _f32(p.weights, dev) for p in parts]
        self.array = (_hip.isi_warp_part * len(parts))()
        for a, p, c, r, w in zip(self.array, parts, self.codes, self.rows, self.weights):
            a.codes, a.rows, a.weights = c.view.data_ptr(), r.view.data_ptr(), None if w is None else w.view.data_ptr()
            a.F, a.r, a.K = p.F, p.r, p.K

    def intact(self):
        buffers = self.codes + self.rows + [w for w in self.weights if w is not None]
        same = all(np.array_equal(c.view.cpu().numpy().view(np.uint16), p.codes) for c, p in zip(self.codes, self.parts))
        return same and all(b.intact() for b in buffers)                                # streamed, never written


def _search(lib, dev, parts, lo, hi, allowed=None, shift=0, rows_shift=0, want_end=True):
    """One isi_code_warp_search_f32 call on guarded buffers -> (dist float32 [Q, N], end int32 [Q, N]); margins asserted."""
    N, T, W, Q, _ = WS.grid(parts)
    device = _Device(parts, dev, shift, rows_shift)
    d_allowed = None if allowed is None else torch.from_numpy(np.ascontiguousarray(allowed, dtype=np.uint8)).to(dev)
    g_dist = _Guarded((Q, N), torch.float32, SENTINEL_F, dev)
    g_end = _Guarded((Q, N), torch.int32, SENTINEL_I, dev)
    rc = lib.isi_code_warp_search_f32(device.array, len(parts), None if d_allowed is None else d_allowed.data_ptr(),
                                      g_dist.view.data_ptr(), g_end.view.data_ptr() if want_end else None, N, T, W, lo, hi, Q,
                                      None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert g_dist.intact() and g_end.intact() and device.intact()
    if not want_end:
        assert bool((g_end.view == SENTINEL_I).all())
    return g_dist.view.cpu().numpy(), g_end.view.cpu().numpy()


def _paths(lib, dev, parts, items, lo, hi):
    """One isi_code_warp_path_f32 call on guarded buffers -> (path int32 [Q, M, W], dist float32 [Q, M])."""
    N, T, W, Q, _ = WS.grid(parts)
    M = items.shape[1]
    device = _Device(parts, dev)
    d_items = torch.from_numpy(np.ascontiguousarray(items, dtype=np.int64)).to(dev)
    g_path = _Guarded((Q, M, W), torch.int32, SENTINEL_I, dev)
    g_dist = _Guarded((Q, M), torch.float32, SENTINEL_F, dev)
    need = lib.isi_code_warp_path_workspace_bytes(M, W, lo, hi, Q)
    assert need == -(-Q * M * W * (hi - lo + 1) // 16) * 16
    g_ws = _Guarded((need,), torch.uint8, 0xA5, dev)
    rc = lib.isi_code_warp_path_f32(device.array, len(parts), d_items.data_ptr(), M, g_path.view.data_ptr(), g_dist.view.data_ptr(),
                                    g_ws.view.data_ptr(), need, N, T, W, lo, hi, Q, None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert g_path.intact() and g_dist.intact() and g_ws.intact() and device.intact()
    return g_path.view.cpu().numpy(), g_dist.view.cpu().numpy()


def _lib():
    from interactive_spectrogram_inpainting import _hip
    return _hip.lib(), _dev()


# ------------------------------------------------------------------------------------- three checks for every geometry
@pytest.mark.parametrize("name", IDS)
def test_exact_on_integer_rows(name):
    """Integer rows in [0, 255], 0/1 weights, NaN and inf rows under the zero weights, sums below 2^24: the int64
    specification exactly, distances and end columns; the same from misaligned codes and rows and without `end`."""
    lib, dev = _lib()
    _, N, T, W, lo, hi, Q, _ = geometry(name)
    parts = list(parts_of(name, True))
    want, want_end, _ = reference(name, True)
    got, end = _search(lib, dev, parts, lo, hi)
    assert np.isfinite(got).all() and np.array_equal(got.astype(np.int64), want) and np.array_equal(end, want_end)
    off, off_end = _search(lib, dev, parts, lo, hi, shift=1, rows_shift=1)
    assert np.array_equal(_bits(off), _bits(got)) and np.array_equal(off_end, end)
    assert np.array_equal(_bits(_search(lib, dev, parts, lo, hi, want_end=False)[0]), _bits(got))


@pytest.mark.parametrize("name", IDS)
def test_float_rows_equal_the_emulation_bit_for_bit_inside_the_bound(name):
    lib, dev = _lib()
    _, N, T, W, lo, hi, Q, _ = geometry(name)
    parts = list(parts_of(name, False))
    emulated, emulated_end, _ = reference(name, False)
    got, end = _search(lib, dev, parts, lo, hi)
    want = reference64(name)
    err, bound = np.abs(got.astype(np.float64) - want), WS.bound(want, parts)
    print(f"warp search {name}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert np.array_equal(_bits(got), _bits(emulated)) and np.array_equal(end, emulated_end)
    assert (err <= bound).all()


def test_null_weights_count_every_cell():
    lib, dev = _lib()
    _, N, T, W, lo, hi, Q, _ = geometry("two-layers")
    rng = np.random.default_rng(9)
    parts = [WS.Part(p.codes, rng.integers(0, 256, p.rows.shape).astype(np.float32), None, p.r) for p in parts_of("two-layers", True)]
    want, want_end, _ = WS.search_int(parts, lo, hi)
    got, end = _search(lib, dev, parts, lo, hi)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(end, want_end)


# ------------------------------------------------------------------------------------------------------- the contract
def test_bits_do_not_depend_on_the_database_the_batch_or_the_alignment():
    lib, dev = _lib()
    _, N, T, W, lo, hi, Q, _ = geometry("two-layers")
    parts = list(parts_of("two-layers", False))
    full, full_end = _search(lib, dev, parts, lo, hi)
    assert np.array_equal(_bits(full), _bits(_search(lib, dev, parts, lo, hi)[0]))     # the run
    order = np.random.default_rng(1).permutation(N)
    moved = [WS.Part(p.codes[order], p.rows, p.weights, p.r) for p in parts]
    got, end = _search(lib, dev, moved, lo, hi)
    assert np.array_equal(_bits(got), _bits(full[:, order])) and np.array_equal(end, full_end[:, order])
    few = [WS.Part(p.codes[100:137], p.rows, p.weights, p.r) for p in parts]           # another N, another place in the grid
    assert np.array_equal(_bits(_search(lib, dev, few, lo, hi)[0]), _bits(full[:, 100:137]))
    for j in range(Q):                                                # another Q
        one = [WS.Part(p.codes, p.rows[j:j + 1], p.weights[j:j + 1], p.r) for p in parts]
        assert np.array_equal(_bits(_search(lib, dev, one, lo, hi)[0][0]), _bits(full[j]))
    for shift, rows_shift in ((1, 0), (3, 1), (0, 2)):
        got, end = _search(lib, dev, parts, lo, hi, shift=shift, rows_shift=rows_shift)
        assert np.array_equal(_bits(got), _bits(full)) and np.array_equal(end, full_end)


def _shift_rows_search(lib, dev, codes, rows, w, W, shift0, step, count, prefill=None):
    N, F, T = codes.shape
    Q, K = rows.shape[0], rows.shape[2]
    d_codes = torch.from_numpy(np.ascontiguousarray(codes).view(np.int16)).to(dev)
    d_rows, d_w = torch.from_numpy(rows).to(dev), torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
    dist = torch.empty(Q, count, N, dtype=torch.float32, device=dev)
    if prefill is not None:
        dist.copy_(torch.from_numpy(prefill))
    need = lib.isi_code_shift_search_workspace_bytes(N, F, T, W, count, K, Q)
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    rc = lib.isi_code_shift_search_rows_f32(d_codes.data_ptr(), d_rows.data_ptr(), d_w.data_ptr(), dist.data_ptr(), N, F, T, W,
                                            shift0, step, count, K, Q, int(prefill is not None), ws.data_ptr(), need, None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    return dist.cpu().numpy()


def test_closed_band_against_the_shifted_search():
    """lo == hi == o: exactly `code_shift_search_spec.search_int` at offset o in the integer regime; on float rows both
    kernels lie within their bounds of the same float64 sum, two layers included."""
    lib, dev = _lib()
    rng = np.random.default_rng(23)
    N, F, T, W, K, Q = 270, 3, 12, 7, 9, 2
    codes = rng.integers(0, K, (N, F, T)).astype(np.uint16)
    query = rng.integers(0, K + 1, (Q, F, W)).astype(np.uint16)                        # K: the mask token
    table = rng.integers(0, 256, (K, K)).astype(np.float32)
    w = (rng.random((Q, F, W)) < 0.7).astype(np.float32)
    gathered = R.gather_rows(table, query.reshape(Q, -1))
    part = WS.Part(codes, gathered, R.mask_token_weights(query, w, K))
    want = SH.search_int(codes, query, w, table, 0, 1, T - W + 1)
    for o in (0, 3, T - W):
        got, end = _search(lib, dev, [part], o, o)
        assert np.array_equal(got.astype(np.int64), want[:, o]) and (end == o + W - 1).all()
    # float rows, top and bottom: warp = the float64 sum within (V + W + 2) u, shifted = within (F W + 2) u per layer
    _, N, T, W, lo, hi, Q, _ = geometry("two-layers")
    top, bottom = parts_of("two-layers", False)
    for o in (0, 2):
        got = _search(lib, dev, [top, bottom], o, o)[0].astype(np.float64)
        want64 = WS.search64([top, bottom], o, o)
        assert (np.abs(got - want64) <= WS.bound(want64, [top, bottom])).all()
        first = _shift_rows_search(lib, dev, top.codes, top.rows, top.weights, W, o, 1, 1)
        both = _shift_rows_search(lib, dev, bottom.codes, bottom.rows, bottom.weights, 2 * W, 2 * o, 2, 1, prefill=first)
        _, mag_t = R.shift_search64(top.codes, top.rows, top.weights, W, o, 1, 1)
        _, mag_b = R.shift_search64(bottom.codes, bottom.rows, bottom.weights, 2 * W, 2 * o, 2, 1)
        slack = R.shift_bound(mag_t, top.F, W)[:, 0] + R.shift_bound(mag_b, bottom.F, 2 * W)[:, 0] + 2 * WS.U * want64
        assert (np.abs(both[:, 0].astype(np.float64) - want64) <= slack).all()
        assert (np.abs(both[:, 0].astype(np.float64) - got) <= slack + WS.bound(want64, [top, bottom])).all()


def test_wider_bands_never_increase_a_distance():
    lib, dev = _lib()
    parts = list(parts_of("ragged-clipped", False))
    bands = [(1, 1), (0, 2), (-2, 3), (-6, 5)]
    dists = [_search(lib, dev, parts, lo, hi)[0] for lo, hi in bands]
    for (lo, hi), got in zip(bands, dists):
        assert np.array_equal(_bits(got), _bits(WS.emulate(parts, lo, hi)[0]))
    for narrow, wide in zip(dists, dists[1:]):
        assert (wide <= narrow).all()
    assert (dists[-1] < dists[0]).any()


def test_allowed_items_and_the_rest():
    lib, dev = _lib()
    _, N, T, W, lo, hi, Q, _ = geometry("ragged-clipped")
    parts = list(parts_of("ragged-clipped", False))
    allowed = (np.arange(N) % 3 != 1).astype(np.uint8)
    got, end = _search(lib, dev, parts, lo, hi, allowed=allowed)
    want, want_end, _ = reference("ragged-clipped", False)
    ok = allowed == 1
    assert np.isposinf(got[:, ~ok]).all() and (end[:, ~ok] == -1).all() and (~ok).any()
    assert np.array_equal(_bits(got[:, ok]), _bits(want[:, ok])) and np.array_equal(end[:, ok], want_end[:, ok])


# ---------------------------------------------------------------------------------------------------------- the paths
@pytest.mark.parametrize("name", ["ragged-clipped", "w-beyond-t", "widest-band", "two-layers", "real"])
def test_paths_equal_the_emulation_and_their_distances_the_search(name):
    lib, dev = _lib()
    _, N, T, W, lo, hi, Q, _ = geometry(name)
    for integer in (True, False):                                     # integer rows tie: the tie rule shows
        parts = list(parts_of(name, integer))
        want_dist, want_end, want_path = reference(name, integer)
        rng = np.random.default_rng(N)
        M = min(N, 64)
        items = np.stack([rng.permutation(N)[:M] for _ in range(Q)])
        items[0, 0], items[-1, M - 1] = N - 1, 0
        path, dist = _paths(lib, dev, parts, items, lo, hi)
        searched = _search(lib, dev, parts, lo, hi)[0]
        for j in range(Q):
            assert np.array_equal(_bits(dist[j]), _bits(searched[j, items[j]]))
            assert np.array_equal(path[j], want_path[j, items[j]])
            assert np.array_equal(path[j, :, -1], want_end[j, items[j]])
            assert all(WS.path_admissible(p, T, lo, hi) for p in path[j])
        if not integer:
            assert np.array_equal(_bits(dist), _bits(np.take_along_axis(want_dist, items, 1)))


def test_paths_of_items_outside_the_database():
    lib, dev = _lib()
    _, N, T, W, lo, hi, Q, _ = geometry("ragged-clipped")
    parts = list(parts_of("ragged-clipped", True))
    items = np.array([[5, -1, N, 7], [0, 1 << 40, 2, -(1 << 40)]], np.int64)
    path, dist = _paths(lib, dev, parts, items, lo, hi)
    bad = (items < 0) | (items >= N)
    assert np.isposinf(dist[bad]).all() and (path[bad] == -1).all()
    want = reference("ragged-clipped", True)[2]
    for j, m in zip(*np.nonzero(~bad)):
        assert np.array_equal(path[j, m], want[j, items[j, m]])


def test_planted_warp_is_found_at_distance_zero():
    """Items that hold the query's columns along a path inside the band -- holds, steps and skips -- are at distance exactly
    0 with that path; the shifted search at every offset is not."""
    lib, dev = _lib()
    rng = np.random.default_rng(31)
    N, F, T, W, K = 300, 4, 24, 16, 32
    E = rng.standard_normal((K, 8)).astype(np.float32)
    table = R.rows64(E, E).astype(np.float32)
    assert (np.diag(table) == 0).all() and (table[~np.eye(K, dtype=bool)] > 0).all()
    codes = rng.integers(0, K, (N, F, T)).astype(np.uint16)
    steps = np.array([1, 0, 1, 2, 1, 1, 0, 0, 1, 2, 2, 1, 1, 0, 1])                    # the drift wanders between 0 and 2
    planted = 2 + np.concatenate([[0], np.cumsum(steps)])
    assert WS.path_admissible(planted, T, -1, 3) and len(planted) == W
    ITEM = 123
    query = codes[ITEM][None, :, planted].copy()                      # the item, played along the planted path
    part = WS.Part(codes, R.gather_rows(table, query.reshape(1, -1)), None)
    got, end = _search(lib, dev, [part], -1, 3)
    assert got[0, ITEM] == 0.0 and end[0, ITEM] == planted[-1] and (np.delete(got[0], ITEM) > 0).all()
    path, dist = _paths(lib, dev, [part], np.array([[ITEM]]), -1, 3)
    assert dist[0, 0] == 0.0 and WS.path_admissible(path[0, 0], T, -1, 3)
    assert np.array_equal(codes[ITEM][:, path[0, 0]], query[0])       # the path found reads the query's codes
    w = np.ones((1, F, W), np.float32)
    shifted = _shift_rows_search(lib, dev, codes, part.rows, w, W, 0, 1, T - W + 1)
    assert (shifted[0, :, ITEM] > 0).all()


def test_cabi_refusals_with_a_device_present():
    lib, dev = _lib()
    check_cabi_refusals(lib)


# ------------------------------------------------------------------------------------------------------- end to end
class _Enc:                                      # stands in for sklearn's LabelEncoder
    def __init__(self, classes):
        self.classes = list(classes)

    def transform(self, values):
        return np.array([self.classes.index(v) for v in values])

    def inverse_transform(self, indexes):
        return np.array([self.classes[int(i)] for i in indexes], dtype=object)


def test_search_warped_end_to_end(monkeypatch):
    import inpainting
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.datasets import code_index
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    dev, K = _dev(), 32
    torch.manual_seed(11)
    vq = VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
               num_embeddings=K, resolution_factors={"bottom": 4, "top": 2}).to(dev).eval()
    encoders = {"pitch": _Enc(range(24, 85)), "instrument_family_str": _Enc([f"fam{i}" for i in range(11)])}
    g = torch.Generator().manual_seed(12)
    N, F_t, T_t, F_b, T_b = 200, 8, 16, 16, 32
    top, bottom = torch.randint(0, K, (N, F_t, T_t), generator=g), torch.randint(0, K, (N, F_b, T_b), generator=g)
    # item 57 played with a held and a skipped column: query column i is item column PATH[i]
    ITEM, TWIN = 57, 150
    PATH = torch.tensor([0, 1, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])
    wide = lambda p: (2 * p[:, None] + torch.arange(2)[None, :]).reshape(-1)          # noqa: E731
    q_top, q_bottom = top[ITEM][:, PATH].clone(), bottom[ITEM][:, wide(PATH)].clone()
    top[TWIN], bottom[TWIN] = top[ITEM], bottom[ITEM]
    attrs = {"pitch": torch.arange(N) % 61, "instrument_family_str": torch.arange(N) % 11}
    index = code_index.CodeIndex.from_arrays(top, bottom, attrs, vq, dev, encoders)
    indices, distances = index.search_warped(q_top.to(dev), q_bottom.to(dev), k=3, drift=(-2, 2))
    assert indices.dtype == torch.int64 and distances.dtype == torch.float32
    assert indices.tolist()[:2] == [ITEM, TWIN] and distances.tolist()[:2] == [0.0, 0.0] and float(distances[2]) > 0
    assert float(index.search(q_top.to(dev), q_bottom.to(dev), k=1)[1][0]) > 0         # the aligned search misses it
    paths = index.warp_paths(indices[:2], q_top.to(dev), q_bottom.to(dev), drift=(-2, 2))
    assert paths.dtype == torch.int64 and paths.shape == (2, T_t) and torch.equal(paths[0].cpu(), PATH)
    # the closed band is the aligned search, and one layer alone
    aligned = index.search(q_top.to(dev), q_bottom.to(dev), k=N)
    closed = index.search_warped(q_top.to(dev), q_bottom.to(dev), k=N, drift=(0, 0))
    assert closed[0][:2].tolist() == aligned[0][:2].tolist() and torch.allclose(closed[1], aligned[1], rtol=1e-5)
    assert index.search_warped(q_top.to(dev), k=2, drift=(-2, 2))[0].tolist() == [ITEM, TWIN]
    alone = WS.Part(bottom.numpy().astype(np.uint16), R.gather_rows(index.table("bottom").cpu().numpy(), q_bottom.numpy().reshape(1, -1)))
    got = index.distances_warped(bottom_code=q_bottom.to(dev), drift=(-4, 4))          # bottom alone: drift in bottom columns
    assert got[1] and np.array_equal(_bits(got[0].cpu().numpy()), _bits(WS.emulate([alone], -4, 4)[0]))
    # the specification, bit for bit: two layers, a layer weight, masks, a mask token, three queries, vectors beside codes
    table_t, table_b = index.table("top").cpu().numpy(), index.table("bottom").cpu().numpy()
    three_t = torch.stack([q_top, top[3], top[9]])
    three_b = torch.stack([q_bottom, bottom[3], bottom[9]])
    three_t[1, 2, 3] = K
    mask_top = torch.zeros(3, F_t, T_t, dtype=torch.bool)
    mask_top[2, :, 2:4] = True
    mask_bottom = mask_top.repeat_interleave(2, -2).repeat_interleave(2, -1)
    w_t = R.mask_token_weights(three_t.numpy().reshape(3, -1), (~mask_top).numpy().astype(np.float32).reshape(3, -1), K)
    w_b = (~mask_bottom).numpy().astype(np.float32).reshape(3, -1) * np.float32(0.5)
    spec_parts = [WS.Part(top.numpy().astype(np.uint16), R.gather_rows(table_t, three_t.numpy().reshape(3, -1)),
                          w_t.reshape(3, F_t, T_t), 1),
                  WS.Part(bottom.numpy().astype(np.uint16), R.gather_rows(table_b, three_b.numpy().reshape(3, -1)),
                          w_b.reshape(3, F_b, T_b), 2)]
    spec, _, spec_path = WS.emulate(spec_parts, -3, 2)
    kw = dict(mask_top=mask_top.to(dev), mask_bottom=mask_bottom.to(dev), layer_weights=(1.0, 0.5), drift=(-3, 2))
    dist, single = index.distances_warped(three_t.to(dev), three_b.to(dev), **kw)
    assert not single and np.array_equal(_bits(dist.cpu().numpy()), _bits(spec))
    indices, distances = index.search_warped(three_t.to(dev), three_b.to(dev), k=5, **kw)
    assert indices.shape == distances.shape == (3, 5)
    for j in range(3):
        order = np.argsort(spec[j], kind="stable")[:5]
        assert indices[j].tolist() == order.tolist() and distances[j].tolist() == spec[j][order].tolist()
    paths = index.warp_paths(indices, three_t.to(dev), three_b.to(dev), **kw)
    assert paths.shape == (3, 5, T_t)
    for j in range(3):
        assert np.array_equal(paths[j].cpu().numpy(), spec_path[j, indices[j].cpu().numpy()])
    v_b = vq.quantize_b.embed_code(three_b.to(dev))                   # vectors that are codebook rows: the same bits
    soft = index.distances_warped(three_t.to(dev), bottom_vectors=v_b, **kw)[0]
    assert torch.equal(soft, dist)
    monkeypatch.setattr(code_index, "ROWS_BUDGET_BYTES", F_b * T_b * K * 4)            # one query at a time
    assert torch.equal(index.distances_warped(three_t.to(dev), three_b.to(dev), **kw)[0], dist)
    assert torch.equal(index.warp_paths(indices, three_t.to(dev), three_b.to(dev), **kw), paths)
    monkeypatch.undo()
    # constraints, exclude, windows
    found = index.search_warped(q_top.to(dev), q_bottom.to(dev), k=2, drift=(-2, 2), attribute_constraints={"instrument_family_str": "fam2"})
    assert found[0].tolist()[0] == ITEM and all(i % 11 == 2 for i in found[0].tolist())
    assert index.search_warped(q_top.to(dev), q_bottom.to(dev), k=1, drift=(-2, 2), exclude=[ITEM])[0].tolist() == [TWIN]
    with pytest.raises(LookupError):
        index.search_warped(q_top.to(dev), attribute_constraints={"pitch": 1000})
    window = index.search_warped(q_top[:, 4:10].to(dev), q_bottom[:, 8:20].to(dev), k=2, drift=(3, 6))
    assert window[0].tolist() == [ITEM, TWIN] and window[1].tolist() == [0.0, 0.0]     # query columns 4 .. 9 = item columns 3, 5 .. 9
    with pytest.raises(_hip.HipLibraryError):
        index.search_warped(q_top, q_bottom)
    # similar_sounds_warped and paste_warped: a hole in the warped sound is filled with the item's own codes
    sound_top, sound_bottom = q_top.unsqueeze(0).clone(), q_bottom.unsqueeze(0).clone()
    hole = torch.zeros(1, F_t, T_t, dtype=torch.bool)
    hole[0, :, 6:9] = True
    damaged_top, damaged_bottom = sound_top.clone(), sound_bottom.clone()
    damaged_top[0, :, 6:9] = (damaged_top[0, :, 6:9] + 1) % K
    damaged_bottom[0, :, 12:18] = (damaged_bottom[0, :, 12:18] + 1) % K
    found = inpainting.similar_sounds_warped(index, damaged_top.to(dev), damaged_bottom.to(dev), mask=hole, k=3, drift=(-2, 2))
    assert [f[2] for f in found[:2]] == [0.0, 0.0] and found[2][2] > 0 and found[0][1] == index.decoded_attributes(ITEM)
    (f_top, f_bottom), _, _ = found[0]
    assert torch.equal(f_top.cpu(), top[ITEM:ITEM + 1]) and torch.equal(f_bottom.cpu(), bottom[ITEM:ITEM + 1])
    assert inpainting.similar_sounds_warped(index, damaged_top.to(dev), damaged_bottom.to(dev), k=1, drift=(-2, 2))[0][2] > 0
    path = index.warp_paths([ITEM], damaged_top[0].to(dev), damaged_bottom[0].to(dev), mask_top=hole.to(dev),
                            mask_bottom=hole.repeat_interleave(2, -2).repeat_interleave(2, -1).to(dev), drift=(-2, 2))
    assert path.shape == (1, T_t)
    mended = inpainting.paste_warped(damaged_top, damaged_bottom, f_top, f_bottom, hole, 0, path[0])
    assert torch.equal(mended[0], sound_top) and torch.equal(mended[1], sound_bottom)
