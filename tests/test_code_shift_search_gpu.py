"""GPU tests of the shift-invariant code search (csrc/code_shift_search.hip) through the C-ABI and through
`CodeIndex.search_shifted`, against the float64 / int64 specification tests/code_shift_search_spec.py: exact searches on
integer tables over every route of the kernel, the derived bound and the fp32 emulation bit for bit on float tables,
bit-identity with `isi_code_search_f32` at W == T and under every change of the launch, the best-offset pass, sentinel
margins around every buffer the kernels write or stream, and `search_shifted`, `similar_fragments`, `patch_from_database`
on a small index."""
import functools

import numpy as np
import pytest
import torch

import code_search_spec as S
import code_shift_search_spec as SS

pytestmark = pytest.mark.gpu

MARGIN = 64                 # sentinel elements on each side of a guarded buffer (keeps 16-byte alignment of the payload)
SENTINEL_F = -12345.0
SENTINEL_U = 0x5A5A
SENTINEL_I = -777

#          N,   F,  T,   W, shift0, step, S,  K,   Q
SHAPES = [(1, 1, 1, 1, 0, 1, 1, 2, 1),                 # smallest case
          (1000, 16, 64, 16, 0, 1, 49, 512, 1),        # top geometry
          (257, 32, 128, 32, 0, 2, 49, 512, 2),        # bottom geometry, step 2
          (1031, 7, 11, 5, 1, 1, 6, 300, 3),           # odd row pitch, W % 8 != 0, shift0 > 0, K % 4 != 0
          (64, 1, 300, 257, 0, 1, 44, 64, 1),          # a second run of one cell
          (64, 2, 200, 8, 0, 1, 193, 64, 1),           # many more offsets than one block or pass
          (50, 4, 12, 4, 0, 1, 9, 4100, 1),            # chunk below 8 cells
          (100, 3, 40, 40, 0, 1, 1, 600, 1)]           # W == T


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


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


def _shift_search(lib, dev, codes, query, w, table, shift0, step, count, prefill=None, shift=0):
    """One isi_code_shift_search_f32 call on guarded buffers -> dist [Q, S, N] float32 (numpy); margins asserted."""
    N, F, T = codes.shape
    Q, W, K = query.shape[0], query.shape[2], table.shape[0]
    g_codes = _u16(codes, dev, shift)
    g_query = _u16(query, dev)
    d_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
    d_table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(dev)
    g_dist = _Guarded((Q, count, N), torch.float32, SENTINEL_F, dev)
    if prefill is not None:
        g_dist.view.copy_(torch.from_numpy(np.ascontiguousarray(prefill, dtype=np.float32)))
    need = lib.isi_code_shift_search_workspace_bytes(N, F, T, W, count, K, Q)
    runs = -(-F * W // 256)
    assert need == (runs * Q * count * N * 4 if runs > 1 else 16)
    g_ws = _Guarded((need // 4,), torch.float32, SENTINEL_F, dev)
    rc = lib.isi_code_shift_search_f32(g_codes.view.data_ptr(), g_query.view.data_ptr(), None if d_w is None else d_w.data_ptr(),
                                       d_table.data_ptr(), g_dist.view.data_ptr(), N, F, T, W, shift0, step, count, K, Q,
                                       int(prefill is not None), g_ws.view.data_ptr(), need, None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert g_dist.intact() and g_ws.intact() and g_codes.intact() and g_query.intact()
    assert np.array_equal(g_codes.view.cpu().numpy().view(np.uint16), codes)          # streamed, never written
    return g_dist.view.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(N, F, T, W, K, Q, seed, integer):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, K, (N, F, T)).astype(np.uint16)
    codes[N - 1, F - 1, T - 1] = K - 1
    codes[0, 0, 0] = K - 1
    query = rng.integers(0, K, (Q, F, W)).astype(np.uint16)
    query[0, F - 1, W - 1] = K - 1
    if integer:
        table = rng.integers(0, 256, (K, K)).astype(np.float32)       # asymmetric: a row / column swap shows
        w = (rng.random((Q, F, W)) < 0.7).astype(np.float32)
        if F * W > 1:
            token = rng.random((Q, F, W)) < 0.15
            token[0, 0, 0], w[0, 0, 0] = True, 1.0                     # a mask-token cell under non-zero weight
            query[token] = K
            assert ((query == K) & (w > 0)).any()
    else:
        table = S.table64(rng.standard_normal((K, 16)).astype(np.float32)).astype(np.float32)
        w = (2.0 * rng.random((Q, F, W))).astype(np.float32)
    return codes, query, w, table                                     # shared among the tests: nobody changes them


@functools.lru_cache(maxsize=None)
def _float_reference(shape):
    N, F, T, W, shift0, step, count, K, Q = shape
    codes, query, w, table = _inputs(N, F, T, W, K, Q, 200 + N, False)
    want, mag = SS.search64(codes, query, w, table, shift0, step, count)
    return want, mag, SS.emulate(codes, query, w, table, shift0, step, count)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_exact_search_on_integer_tables(shape):
    """Integer table in [0, 255], 0/1 weights, every sum <= 255 F W < 2^24: bitwise the int64 specification at every
    offset, with mask-token query cells under non-zero weight; the same from a codes buffer one element off its
    alignment; with null weights; and accumulated onto a prefilled dist."""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    N, F, T, W, shift0, step, count, K, Q = shape
    codes, query, w, table = _inputs(N, F, T, W, K, Q, 100 + N, True)
    want = SS.search_int(codes, query, w, table, shift0, step, count)
    assert want.max() + 1000 < 2 ** 24 and want.shape == (Q, count, N)
    got = _shift_search(lib, dev, codes, query, w, table, shift0, step, count)
    assert np.array_equal(got.astype(np.int64), want)
    off = _shift_search(lib, dev, codes, query, w, table, shift0, step, count, shift=1)
    assert np.array_equal(off.view(np.uint32), got.view(np.uint32))
    prefill = np.random.default_rng(N).integers(0, 1000, (Q, count, N)).astype(np.float32)
    got = _shift_search(lib, dev, codes, query, w, table, shift0, step, count, prefill=prefill)
    assert np.array_equal(got.astype(np.int64), want + prefill.astype(np.int64))
    got = _shift_search(lib, dev, codes, query, None, table, shift0, step, count)
    assert np.array_equal(got.astype(np.int64), SS.search_int(codes, query, None, table, shift0, step, count))


@pytest.mark.parametrize("shape", SHAPES[:5], ids=lambda s: "-".join(map(str, s)))
def test_float_search_inside_the_derived_bound(shape):
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    N, F, T, W, shift0, step, count, K, Q = shape
    codes, query, w, table = _inputs(N, F, T, W, K, Q, 200 + N, False)
    want, mag, emulated = _float_reference(shape)
    got = _shift_search(lib, dev, codes, query, w, table, shift0, step, count)
    err, bound = np.abs(got.astype(np.float64) - want), SS.bound(mag, F, W)
    print(f"shift search {shape}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all()
    # and bit for bit the fp32 emulation of the documented summation order
    assert np.array_equal(got.view(np.uint32), emulated.view(np.uint32))


@pytest.mark.parametrize("N,F,T,K,Q", [(100, 3, 40, 600, 1), (300, 16, 64, 512, 2), (70, 7, 11, 300, 2)])
def test_full_width_equals_the_aligned_search_bit_for_bit(N, F, T, K, Q):
    """W == T, S == 1, shift0 == 0: the bits of isi_code_search_f32 with C = F * T (one run, four runs, an odd pitch)."""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    codes, query, w, table = _inputs(N, F, T, T, K, Q, 400 + N, False)
    got = _shift_search(lib, dev, codes, query, w, table, 0, 1, 1)
    C = F * T
    d_codes, d_query = (torch.from_numpy(a.view(np.int16)).to(dev) for a in (codes, query))
    d_w, d_table = torch.from_numpy(w).to(dev), torch.from_numpy(table).to(dev)
    dist = torch.empty(Q, N, dtype=torch.float32, device=dev)
    need = lib.isi_code_search_workspace_bytes(N, C, K, Q)
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    assert lib.isi_code_search_f32(d_codes.data_ptr(), d_query.data_ptr(), d_w.data_ptr(), d_table.data_ptr(), None,
                                   dist.data_ptr(), N, C, K, Q, 0, ws.data_ptr(), need, None) == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(got[:, 0].view(np.uint32), dist.cpu().numpy().view(np.uint32))


def test_deterministic_and_local_to_query_item_and_offset():
    """dist[j][s][n] keeps its bits when N, Q, S, step / shift0 (the same absolute offset), the item's position in the
    launch, the alignment -- and with them the kernel's route and pass structure -- change."""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)          # noqa: E731
    N, F, T, W, K, Q = 700, 16, 64, 16, 512, 3
    codes, query, w, table = _inputs(N, F, T, W, K, Q, 7, False)
    codes = codes.copy()
    codes[500] = codes[20]                                            # the same sound stored twice
    run = lambda c, q, ww, *a, **k: _shift_search(lib, dev, c, q, ww, table, *a, **k)             # noqa: E731
    full = run(codes, query, w, 0, 1, 49)
    assert np.array_equal(bits(full), bits(run(codes, query, w, 0, 1, 49)))
    assert np.array_equal(bits(full[:, :, 500]), bits(full[:, :, 20]))
    assert np.array_equal(bits(run(codes[100:300].copy(), query, w, 0, 1, 49)), bits(full[:, :, 100:300]))
    for j in range(Q):
        assert np.array_equal(bits(run(codes, query[j:j + 1], w[j:j + 1], 0, 1, 49)[0]), bits(full[j]))
    assert np.array_equal(bits(run(codes, query, w, 8, 1, 9)), bits(full[:, 8:17]))          # fewer offsets, one block more
    assert np.array_equal(bits(run(codes, query, w, 3, 1, 5)), bits(full[:, 3:8]))           # a start the vectors cannot take
    assert np.array_equal(bits(run(codes, query, w, 8, 2, 20)), bits(full[:, 8:48:2]))       # step 2
    assert np.array_equal(bits(run(codes, query, w, 1, 3, 16)), bits(full[:, 1:49:3]))       # step 3
    assert np.array_equal(bits(run(codes, query, w, 0, 1, 49, shift=1)), bits(full))         # codes off their alignment
    # four runs (the bottom geometry): step 2 against every column, two passes of offsets against one
    N, F, T, W = 200, 32, 128, 32
    codes, query, w, table = _inputs(N, F, T, W, K, 1, 8, False)
    every = run(codes, query, w, 0, 1, 97)
    assert np.array_equal(bits(run(codes, query, w, 0, 2, 49)), bits(every[:, ::2]))
    assert np.array_equal(bits(run(codes, query, w, 16, 2, 40, shift=1)), bits(every[:, 16:96:2]))


def test_best_offset_ties_allowed_and_margins():
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    Q, count, N = 3, 11, 1031
    rng = np.random.default_rng(5)
    dist = rng.integers(1, 50, (Q, count, N)).astype(np.float32)      # small integers: plenty of natural ties
    dist[0, 2, :] = dist[0, 7, :] = 0.0                               # planted: s = 2 and s = 7 tie everywhere
    dist[1, count - 1, ::2] = dist[1, 0, ::2] = -1.0                  # the first and the last offset tie
    dist[2, count - 1, 5] = -3.0                                      # a unique minimum at the last offset
    allowed = (np.arange(N) % 4 != 1).astype(np.uint8)
    g_dist = _Guarded((Q, count, N), torch.float32, SENTINEL_F, dev)
    g_dist.view.copy_(torch.from_numpy(dist))
    for use in (allowed, None):
        g_best = _Guarded((Q, N), torch.float32, SENTINEL_F, dev)
        g_shift = _Guarded((Q, N), torch.int32, SENTINEL_I, dev)
        d_allowed = None if use is None else torch.from_numpy(use).to(dev)
        rc = lib.isi_code_shift_best_f32(g_dist.view.data_ptr(), None if use is None else d_allowed.data_ptr(),
                                         g_best.view.data_ptr(), g_shift.view.data_ptr(), N, count, Q, None)
        assert rc == 0, lib.isi_last_error()
        torch.cuda.synchronize()
        assert g_best.intact() and g_shift.intact() and g_dist.intact()
        assert np.array_equal(g_dist.view.cpu().numpy(), dist)
        value, shift = SS.best(dist, use)
        got_value, got_shift = g_best.view.cpu().numpy(), g_shift.view.cpu().numpy()
        assert got_shift.dtype == np.int32 and np.array_equal(got_shift, shift)
        assert np.array_equal(got_value.astype(np.float64), value)
        ok = np.ones(N, bool) if use is None else use == 1
        assert (got_shift[0, ok] == 2).all() and (got_shift[1, ok][(np.arange(N) % 2 == 0)[ok]] == 0).all()
        assert got_shift[2, 5] == (count - 1 if ok[5] else -1)
        if use is not None:
            assert np.isposinf(got_value[:, ~ok]).all() and (got_shift[:, ~ok] == -1).all() and (~ok).any()


class _Enc:                                      # stands in for sklearn's LabelEncoder
    def __init__(self, classes):
        self.classes = list(classes)

    def transform(self, values):
        return np.array([self.classes.index(v) for v in values])

    def inverse_transform(self, indexes):
        return np.array([self.classes[int(i)] for i in indexes], dtype=object)


def test_search_shifted_end_to_end(monkeypatch):
    import inpainting
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.datasets import code_index
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    dev = _dev()
    K = 32
    torch.manual_seed(11)
    vq = VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
               num_embeddings=K, resolution_factors={"bottom": 4, "top": 2}).to(dev).eval()
    encoders = {"pitch": _Enc(range(24, 85)), "instrument_family_str": _Enc([f"fam{i}" for i in range(11)])}
    g = torch.Generator().manual_seed(12)
    N, F_t, T_t, F_b, T_b = 200, 8, 16, 16, 32
    top, bottom = torch.randint(0, K, (N, F_t, T_t), generator=g), torch.randint(0, K, (N, F_b, T_b), generator=g)
    ITEM, AT, W = 57, 5, 6
    frag_top, frag_bottom = top[ITEM, :, AT:AT + W].clone(), bottom[ITEM, :, 2 * AT:2 * (AT + W)].clone()
    top[150, :, 2:2 + W], bottom[150, :, 4:4 + 2 * W] = frag_top, frag_bottom          # the same fragment, elsewhere in 150
    attrs = {"pitch": torch.arange(N) % 61, "instrument_family_str": torch.arange(N) % 11}
    index = code_index.CodeIndex.from_arrays(top, bottom, attrs, vq, dev, encoders)
    # an item's own columns as the query: that item, at that offset, at distance exactly 0; ties by item index
    indices, shifts, distances = index.search_shifted(frag_top.to(dev), frag_bottom.to(dev), k=3)
    assert indices.dtype == shifts.dtype == torch.int64 and distances.dtype == torch.float32
    assert indices.tolist()[:2] == [ITEM, 150] and shifts.tolist()[:2] == [AT, 2] and distances.tolist()[:2] == [0.0, 0.0]
    assert float(distances[2]) > 0
    indices, shifts, distances = index.search_shifted(frag_top.to(dev), k=2)           # the top layer alone
    assert indices.tolist() == [ITEM, 150] and shifts.tolist() == [AT, 2] and distances.tolist() == [0.0, 0.0]
    indices, shifts, distances = index.search_shifted(bottom_code=frag_bottom.to(dev), k=2)       # bottom alone: bottom columns
    assert indices.tolist() == [ITEM, 150] and shifts.tolist() == [2 * AT, 4] and distances.tolist() == [0.0, 0.0]
    # two layers, a layer weight, masks, three queries: the specification's top + bottom, bit for bit, at every offset
    q_top = torch.stack([frag_top, top[3, :, 1:1 + W], top[9, :, 10:10 + W]])
    q_bottom = torch.stack([frag_bottom, bottom[3, :, 2:2 + 2 * W], bottom[9, :, 20:20 + 2 * W]])
    q_top[1, 2, 3] = K                                               # the prior's mask token: counts nothing
    mask_top = torch.zeros(3, F_t, W, dtype=torch.bool)
    mask_top[2, :, 2:4] = True
    mask_bottom = mask_top.repeat_interleave(2, -2).repeat_interleave(2, -1)
    table_t, table_b = index.table("top").cpu().numpy(), index.table("bottom").cpu().numpy()
    w_t = (~mask_top).numpy().astype(np.float32)
    w_b = (~mask_bottom).numpy().astype(np.float32) * np.float32(0.5)
    S_all = T_t - W + 1
    spec = SS.emulate(top.numpy(), q_top.numpy(), w_t, table_t, 0, 1, S_all) \
        + SS.emulate(bottom.numpy(), q_bottom.numpy(), w_b, table_b, 0, 2, S_all)
    assert spec.dtype == np.float32
    kw = dict(mask_top=mask_top.to(dev), mask_bottom=mask_bottom.to(dev), layer_weights=(1.0, 0.5))
    dist = index.distances_shifted(q_top.to(dev), q_bottom.to(dev), **kw)
    assert dist.shape == (3, S_all, N) and np.array_equal(dist.cpu().numpy().view(np.uint32), spec.view(np.uint32))

    def ranking(d, first, allowed, k):
        """The specification's answer from dist [S', N] whose first offset is `first`: (indices, shifts, distances)."""
        value, shift = SS.best(d[None], allowed)
        order = np.argsort(value[0], kind="stable")[:min(k, N if allowed is None else int(allowed.sum()))]
        return order.tolist(), (shift[0][order] + first).tolist(), value[0][order].astype(np.float32).tolist()
    indices, shifts, distances = index.search_shifted(q_top.to(dev), q_bottom.to(dev), k=5, **kw)
    assert indices.shape == shifts.shape == distances.shape == (3, 5)
    for j in range(3):
        assert (indices[j].tolist(), shifts[j].tolist(), distances[j].tolist()) == ranking(spec[j], 0, None, 5)
    # the grouping of the queries changes nothing (a budget that takes one query at a time)
    monkeypatch.setattr(code_index, "SHIFT_BUDGET_BYTES", S_all * N * 4)
    again = index.search_shifted(q_top.to(dev), q_bottom.to(dev), k=5, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, (indices, shifts, distances)))
    assert torch.equal(index.distances_shifted(q_top.to(dev), q_bottom.to(dev), **kw), dist)
    monkeypatch.undo()
    # shift_range, attribute_constraints, exclude: every returned item and shift is allowed, and the answer is the spec's
    cases = [dict(shift_range=(3, 9)), dict(shift_range=(9, 100)), dict(shift_range=(5, 6)),
             dict(attribute_constraints={"instrument_family_str": "fam2"}),        # 57 % 11 = 2: the item itself is allowed
             dict(attribute_constraints={"instrument_family_str": "fam7"}, shift_range=(1, 4)),
             dict(exclude=[ITEM, 150]), dict(exclude=[ITEM], shift_range=(0, 2), attribute_constraints={"pitch_class": 0})]
    for case in cases:
        lo, hi = case.get("shift_range", (0, S_all))
        hi = min(hi, S_all)
        allowed = index.allowed(case.get("attribute_constraints"), case.get("exclude"))
        allowed = None if allowed is None else allowed.cpu().numpy()
        got = index.search_shifted(q_top[0].to(dev), q_bottom[0].to(dev), k=7, **case)
        assert len(got[0]) == min(7, N if allowed is None else int(allowed.sum())) and len(got[0]) > 0, case
        assert all(lo <= o < hi for o in got[1].tolist()), case
        assert allowed is None or all(allowed[i] == 1 for i in got[0].tolist()), case
        assert not set(got[0].tolist()) & set(case.get("exclude", [])), case
        plain = SS.emulate(top.numpy(), q_top[:1].numpy(), None, table_t, lo, 1, hi - lo) \
            + SS.emulate(bottom.numpy(), q_bottom[:1].numpy(), None, table_b, 2 * lo, 2, hi - lo)
        assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == ranking(plain[0], lo, allowed, 7), case
    assert index.search_shifted(q_top[0].to(dev), q_bottom[0].to(dev), shift_range=(5, 6))[0][0] == ITEM
    with pytest.raises(LookupError):
        index.search_shifted(q_top[0].to(dev), attribute_constraints={"pitch": 1000})
    with pytest.raises(_hip.HipLibraryError):
        index.search_shifted(q_top[0], q_bottom[0])
    # similar_fragments: a sound that carries the fragment at columns 3 .. 8, with two of its columns to be regenerated
    sound_top, sound_bottom = torch.randint(0, K, (1, F_t, 12), generator=g), torch.randint(0, K, (1, F_b, 24), generator=g)
    sound_top[0, :, 3:3 + W], sound_bottom[0, :, 6:6 + 2 * W] = frag_top, frag_bottom
    hole = torch.zeros(1, F_t, W, dtype=torch.bool)
    hole[0, :, 2:4] = True                                            # window columns 2, 3 = sound columns 5, 6
    damaged_top, damaged_bottom = sound_top.clone(), sound_bottom.clone()
    damaged_top[0, :, 5:7], damaged_bottom[0, :, 10:14] = (damaged_top[0, :, 5:7] + 1) % K, (damaged_bottom[0, :, 10:14] + 1) % K
    found = inpainting.similar_fragments(index, damaged_top.to(dev), damaged_bottom.to(dev), 3, W, mask=hole, k=3)
    assert [(f[2], f[3]) for f in found[:2]] == [(0.0, AT), (0.0, 2)] and found[2][2] > 0
    (f_top, f_bottom), f_attrs, _, _ = found[0]
    assert torch.equal(f_top.cpu(), top[ITEM:ITEM + 1]) and torch.equal(f_bottom.cpu(), bottom[ITEM:ITEM + 1])
    assert f_attrs == index.decoded_attributes(ITEM) and f_attrs["instrument_family_str"] == "fam2"
    assert torch.equal(found[1][0][0].cpu(), top[150:151])
    without = inpainting.similar_fragments(index, damaged_top.to(dev), damaged_bottom.to(dev), 3, W, k=1)
    assert without[0][2] > 0                                          # the damaged columns count when nothing masks them
    # patch_from_database: the hole (sound columns 5, 6) with 2 columns of context = the window 3 .. 8 again
    whole = torch.zeros(1, F_t, 12, dtype=torch.bool)
    whole[0, :, 5:7] = True
    patched = inpainting.patch_from_database(index, damaged_top.to(dev), damaged_bottom.to(dev), whole.to(dev), context_top=2, k=2)
    assert [(p[2], p[3]) for p in patched] == [(0.0, AT), (0.0, 2)] and patched[0][1] == index.decoded_attributes(ITEM)
    for (p_top, p_bottom), _, _, shift in patched:
        item = ITEM if shift == AT else 150
        assert torch.equal(p_top.cpu(), sound_top) and torch.equal(p_bottom.cpu(), sound_bottom)      # the fragment is whole again
        assert torch.equal(p_top.cpu()[0, :, 5:7], top[item, :, shift + 2:shift + 4])
        assert torch.equal(p_bottom.cpu()[0, :, 10:14], bottom[item, :, 2 * shift + 4:2 * shift + 8])
    # a partial hole in the bottom layer: only those cells change, and they are the winner's codes at the reported shift
    part = torch.zeros(1, F_b, 24, dtype=torch.bool)
    part[0, 3:9, 11:13] = True
    (p_top, p_bottom), _, distance, shift = inpainting.patch_from_database(index, damaged_top.to(dev), damaged_bottom.to(dev),
                                                                           part.to(dev), layer="bottom", context_top=2, k=1,
                                                                           attribute_constraints={"instrument_family_str": "fam7"})[0]
    start = 11 // 2 - 2                                               # the window: top columns 3 .. 8 (5, 6 hold the hole)
    winner = index.search_shifted(damaged_top[0, :, start:start + 6].to(dev), damaged_bottom[0, :, 2 * start:2 * start + 12].to(dev),
                                  mask_bottom=part[0, :, 2 * start:2 * start + 12].to(dev), k=1,
                                  attribute_constraints={"instrument_family_str": "fam7"})
    assert int(winner[1][0]) == shift and float(winner[2][0]) == distance and int(winner[0][0]) % 11 == 7
    item = int(winner[0][0])
    assert torch.equal(p_top.cpu(), damaged_top)
    want = damaged_bottom.clone()
    want[0, 3:9, 11:13] = bottom[item, 3:9, 11 - 2 * start + 2 * shift:13 - 2 * start + 2 * shift]
    assert torch.equal(p_bottom.cpu(), want)
