"""GPU tests of the code-database search (csrc/code_search.hip) through the C-ABI, with tables the tests build themselves,
against the float64 / int64 specification tests/code_search_spec.py: the table kernel's bound, zero diagonal and bitwise
symmetry; exact searches on integer tables; the derived bound on float tables; determinism and item-locality bit for bit;
sentinel margins around every buffer the kernels write or stream; and `CodeIndex`, `similar_sounds`,
`sample_from_database(similar_to=...)` and the POST form of /sample-from-dataset on the fixture models."""
import json

import numpy as np
import pytest
import torch

import code_search_spec as S

pytestmark = pytest.mark.gpu

MARGIN = 64                 # sentinel elements on each side of a guarded buffer (keeps 16-byte alignment of the payload)
SENTINEL_F = -12345.0
SENTINEL_U = 0x5A5A


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


def _search(lib, dev, codes, query, w, table, allowed=None, prefill=None, shift=0):
    """One isi_code_search_f32 call on guarded buffers -> dist [Q, N] float32 (numpy); the margins are asserted."""
    N, C = codes.shape
    Q, K = query.shape[0], table.shape[0]
    g_codes = _u16(codes, dev, shift)
    g_query = _u16(query, dev)
    d_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
    d_table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(dev)
    d_allowed = None if allowed is None else torch.from_numpy(np.ascontiguousarray(allowed, dtype=np.uint8)).to(dev)
    g_dist = _Guarded((Q, N), torch.float32, SENTINEL_F, dev)
    if prefill is not None:
        g_dist.view.copy_(torch.from_numpy(np.ascontiguousarray(prefill, dtype=np.float32)))
    need = lib.isi_code_search_workspace_bytes(N, C, K, Q)
    assert need == -(-C // 256) * Q * N * 4
    g_ws = _Guarded((need // 4,), torch.float32, SENTINEL_F, dev)
    rc = lib.isi_code_search_f32(g_codes.view.data_ptr(), g_query.view.data_ptr(), None if d_w is None else d_w.data_ptr(),
                                 d_table.data_ptr(), None if d_allowed is None else d_allowed.data_ptr(),
                                 g_dist.view.data_ptr(), N, C, K, Q, int(prefill is not None), g_ws.view.data_ptr(), need, None)
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert g_dist.intact() and g_ws.intact() and g_codes.intact() and g_query.intact()
    assert np.array_equal(g_codes.view.cpu().numpy().view(np.uint16), codes)          # streamed, never written
    return g_dist.view.cpu().numpy()


def _inputs(N, C, K, Q, seed, integer):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, K, (N, C)).astype(np.uint16)
    codes[N - 1, C - 1] = K - 1
    codes[0, 0] = K - 1
    query = rng.integers(0, K, (Q, C)).astype(np.uint16)
    query[0, C - 1] = K - 1
    if integer:
        table = rng.integers(0, 256, (K, K)).astype(np.float32)       # asymmetric: a row / column swap shows
        w = (rng.random((Q, C)) < 0.7).astype(np.float32)
        if C > 1:
            token = rng.random((Q, C)) < 0.15
            token[0, 0], w[0, 0] = True, 1.0                           # a mask-token cell under non-zero weight
            query[token] = K
            assert ((query == K) & (w > 0)).any()
    else:
        table = S.table64(rng.standard_normal((K, 16)).astype(np.float32)).astype(np.float32)
        w = (2.0 * rng.random((Q, C))).astype(np.float32)
    return codes, query, w, table


@pytest.mark.parametrize("K,D", [(512, 64), (300, 64), (7, 3), (1024, 32)])
def test_distance_table_bound_diagonal_symmetry(K, D):
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    E = np.random.default_rng(K + D).standard_normal((K, D)).astype(np.float32)
    d_E = torch.from_numpy(E).to(dev)
    g_T = _Guarded((K, K), torch.float32, SENTINEL_F, dev)
    assert lib.isi_code_distance_table_f32(d_E.data_ptr(), g_T.view.data_ptr(), K, D, None) == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    assert g_T.intact()
    T = g_T.view.cpu().numpy()
    T64 = S.table64(E)
    err, bound = np.abs(T.astype(np.float64) - T64), S.table_bound(T64, D)
    print(f"table K={K} D={D}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert (np.diag(T) == 0).all()
    assert np.array_equal(T.view(np.uint32), T.T.copy().view(np.uint32))


@pytest.mark.parametrize("N,C,K,Q", [(1, 1, 2, 1), (1000, 1024, 512, 1), (257, 4096, 512, 2), (1031, 77, 300, 3),
                                     (64, 1000, 1024, 1)])
def test_exact_search_on_integer_tables(N, C, K, Q):
    """Integer table in [0, 255], 0/1 weights, sums below 2^24: bitwise the int64 specification.  Mask-token query cells
    under non-zero weight count nothing, a third of the items is not allowed (+inf), and a second call accumulates onto
    a prefilled dist."""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    codes, query, w, table = _inputs(N, C, K, Q, 100 + N, integer=True)
    want = S.search_int(codes, query, w, table)
    assert want.max() < 2 ** 24
    allowed = (np.arange(N) % 3 != 1).astype(np.uint8)
    got = _search(lib, dev, codes, query, w, table, allowed=allowed)
    assert np.array_equal(got.astype(np.float64), S.apply_allowed(want, allowed))
    prefill = np.random.default_rng(N).integers(0, 1000, (Q, N)).astype(np.float32)
    got = _search(lib, dev, codes, query, w, table, prefill=prefill)
    assert np.array_equal(got.astype(np.int64), want + prefill.astype(np.int64))
    # null weights: 1 on every cell
    got = _search(lib, dev, codes, query, None, table)
    assert np.array_equal(got.astype(np.int64), S.search_int(codes, query, None, table))


@pytest.mark.parametrize("N,C,K,Q", [(300, 264, 600, 2), (200, 72, 1500, 1), (100, 40, 3000, 1), (50, 16, 4100, 1)])
def test_exact_search_on_every_chunk_size(N, C, K, Q):
    """The chunk of staged cells shrinks with K -- 24 cells at K = 600, 8 at 1500 (codes still read as vectors), 5 at 3000
    and 3 at 4100 (codes read one by one) -- and C = 264 leaves a second run of 8 cells: the same exact answer on each."""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    codes, query, w, table = _inputs(N, C, K, Q, 300 + N, integer=True)
    allowed = (np.arange(N) % 3 != 1).astype(np.uint8)
    got = _search(lib, dev, codes, query, w, table, allowed=allowed)
    assert np.array_equal(got.astype(np.float64), S.apply_allowed(S.search_int(codes, query, w, table), allowed))
    assert np.array_equal(got.view(np.uint32), _search(lib, dev, codes, query, w, table, allowed=allowed, shift=1).view(np.uint32))


@pytest.mark.parametrize("N,C,K,Q", [(1000, 1024, 512, 1), (257, 4096, 512, 2), (1031, 77, 300, 3), (64, 1000, 1024, 1)])
def test_float_search_inside_the_derived_bound(N, C, K, Q):
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    codes, query, w, table = _inputs(N, C, K, Q, 200 + N, integer=False)
    want, mag = S.search64(codes, query, w, table)
    got = _search(lib, dev, codes, query, w, table).astype(np.float64)
    err, bound = np.abs(got - want), S.search_bound(mag, C)
    print(f"search N={N} C={C} K={K} Q={Q}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all()
    # and bit for bit the fp32 emulation of the documented summation order
    assert np.array_equal(got.astype(np.float32).view(np.uint32), S.emulate_f32(codes, query, w, table).view(np.uint32))


def test_deterministic_and_item_local():
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    N, C, K, Q = 1000, 1024, 512, 3
    codes, query, w, table = _inputs(N, C, K, Q, 7, integer=False)
    codes[500] = codes[20]                                            # the same sound stored twice
    bits = lambda a: a.view(np.uint32)                                # noqa: E731
    full = _search(lib, dev, codes, query, w, table)
    assert np.array_equal(bits(full), bits(_search(lib, dev, codes, query, w, table)))
    assert np.array_equal(bits(full[:, 500]), bits(full[:, 20]))
    alone = _search(lib, dev, codes[100:200].copy(), query, w, table)
    assert np.array_equal(bits(alone), bits(full[:, 100:200].copy()))
    for j in range(Q):
        one = _search(lib, dev, codes, query[j:j + 1], w[j:j + 1], table)
        assert np.array_equal(bits(one[0]), bits(full[j]))
    # the route the codes are read by (16-byte vectors / one by one, picked from the base's alignment) changes no bit
    assert np.array_equal(bits(full), bits(_search(lib, dev, codes, query, w, table, shift=1)))


class _Enc:                                      # stands in for sklearn's LabelEncoder
    def __init__(self, classes):
        self.classes = list(classes)

    def transform(self, values):
        return np.array([self.classes.index(v) for v in values])

    def inverse_transform(self, indexes):
        return np.array([self.classes[int(i)] for i in indexes], dtype=object)


def test_code_index_end_to_end(golden_dir):
    import flask_server
    import inpainting
    from test_prior_gpu import _models
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.datasets.code_index import CodeIndex
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    _, top_prior, bottom_prior = _models(golden_dir)
    dev = _dev()
    K = int(top_prior.n_class)
    assert K == int(bottom_prior.n_class) == 32
    torch.manual_seed(11)
    vq = VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
               num_embeddings=K, resolution_factors={"bottom": 4, "top": 2}).to(dev).eval()
    encoders = {"pitch": _Enc(range(24, 85)), "instrument_family_str": _Enc([f"fam{i}" for i in range(11)])}
    g = torch.Generator().manual_seed(12)
    N, COPY = 500, 124
    top, bottom = torch.randint(0, K, (N, 8, 4), generator=g), torch.randint(0, K, (N, 16, 8), generator=g)
    top[300], bottom[300] = top[40], bottom[40]
    top[COPY], bottom[COPY] = top[40], bottom[40]
    changed = [(0, 0), (2, 1), (3, 3), (5, 2), (7, 0)]
    for f, t in changed:
        top[COPY, f, t] = (top[40, f, t] + 1 + 3 * f) % K
    attrs = {"pitch": torch.arange(N) % 61, "instrument_family_str": torch.arange(N) % 11}
    index = CodeIndex.from_arrays(top, bottom, attrs, vq, dev, encoders)
    assert index.top.dtype == torch.uint16 and index.top.is_cuda and len(index) == N
    q_top, q_bottom = top[40].to(dev), bottom[40].to(dev)
    # the tables are the kernel's, from the VQ-VAE's codebooks; they follow the buffer
    T_top = index.table("top").cpu().numpy()
    E = vq.quantize_t.embed.detach().t().cpu().numpy()
    T64 = S.table64(E)
    assert (np.abs(T_top - T64) <= S.table_bound(T64, 16)).all() and index.table("top") is index.table("top")
    indices, distances = index.search(q_top, q_bottom, k=3)
    assert indices.dtype == torch.int64 and distances.dtype == torch.float32
    assert indices.tolist() == [40, 300, COPY] and distances[:2].tolist() == [0.0, 0.0]
    terms = [float(T_top[int(top[40, f, t]), int(top[COPY, f, t])]) for f, t in changed]
    d64 = float(np.sum(np.float64(terms)))
    assert d64 > 0 and abs(float(distances[2]) - d64) <= S.search_bound(np.sum(np.abs(terms)), 32)
    # the five changed cells masked out: three exact ties, in index order
    hole = torch.zeros(8, 4, dtype=torch.bool, device=dev)
    for f, t in changed:
        hole[f, t] = True
    indices, distances = index.search(q_top, q_bottom, mask_top=hole, k=3)
    assert indices.tolist() == [40, COPY, 300] and distances.tolist() == [0.0, 0.0, 0.0]
    # a query straight from an inpainting request: the prior's mask token (index K) under the hole, no mask given
    holed = torch.where(hole, torch.full_like(q_top, K), q_top)
    indices, distances = index.search(holed.unsqueeze(0), q_bottom.unsqueeze(0), k=3)
    assert indices.tolist() == [40, COPY, 300] and distances.tolist() == [0.0, 0.0, 0.0]
    # constraints and exclusions (40 % 11 = 7; 300 % 11 = 124 % 11 = 3)
    indices, _ = index.search(q_top, q_bottom, k=2, attribute_constraints={"instrument_family_str": "fam3"})
    assert indices.tolist() == [300, COPY]
    indices, _ = index.search(q_top, q_bottom, k=2, exclude=[40])
    assert indices.tolist() == [300, COPY]
    indices, distances = index.search(q_top, q_bottom, k=8, attribute_constraints={"pitch": 24 + 40, "instrument_family_str": "fam7"})
    assert indices.tolist() == [40] and distances.tolist() == [0.0]      # 40 is the only item with both (lcm 671 > N)
    with pytest.raises(LookupError):
        index.search(q_top, q_bottom, attribute_constraints={"pitch": 1000})
    # top layer alone, a layer weight, and the batched form
    indices, distances = index.search(q_top, k=2)
    assert indices.tolist() == [40, 300]
    both, d_both = index.search(torch.stack([q_top, top[7].to(dev)]), torch.stack([q_bottom, bottom[7].to(dev)]), k=2,
                                layer_weights=(1.0, 0.5))
    assert both.shape == (2, 2) and both[0].tolist() == [40, 300] and int(both[1, 0]) == 7 and d_both[:, 0].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        index.search(q_top[:, :3])
    with pytest.raises(_hip.HipLibraryError):
        index.search(q_top.cpu(), q_bottom.cpu())
    # the table follows the codebook buffer
    before = index.table("top")
    vq.quantize_t.embed.mul_(2.0)
    after = index.table("top")
    assert after is not before and torch.equal(after, before * 4.0)
    vq.quantize_t.embed.mul_(0.5)
    # similar_sounds: a map longer than the window (the window starts at column 2) ...
    long_top = torch.cat([torch.randint(0, K, (1, 8, 2), generator=g), top[40:41], torch.randint(0, K, (1, 8, 1), generator=g)], -1).to(dev)
    long_bottom = torch.cat([torch.randint(0, K, (1, 16, 4), generator=g), bottom[40:41], torch.randint(0, K, (1, 16, 2), generator=g)], -1).to(dev)
    found = inpainting.similar_sounds(index, long_top, long_bottom, start_index_top=2, k=3)
    assert [f[2] for f in found[:2]] == [0.0, 0.0] and found[2][2] > 0
    (f_top, f_bottom), f_attrs, _ = found[0]
    assert torch.equal(f_top.cpu(), top[40:41]) and torch.equal(f_bottom.cpu(), bottom[40:41])
    assert f_attrs == {"pitch": 64, "instrument_family_str": "fam7", "pitch_class": 4, "octave": 5}
    assert found[1][1]["instrument_family_str"] == "fam3" and torch.equal(found[2][0][0].cpu(), top[COPY:COPY + 1])
    # ... with a top-layer mask over the changed cells (extended to the bottom layer): three ties in index order
    found = inpainting.similar_sounds(index, long_top, long_bottom, mask=hole.unsqueeze(0), layer="top", start_index_top=2, k=3)
    assert [f[2] for f in found] == [0.0, 0.0, 0.0] and torch.equal(found[1][0][0].cpu(), top[COPY:COPY + 1])
    # ... and a map shorter than the stored duration: the columns it is continued with weigh nothing
    short = inpainting.similar_sounds(index, top[40:41, :, :3].to(dev), bottom[40:41, :, :6].to(dev), k=2)
    assert [f[2] for f in short] == [0.0, 0.0] and torch.equal(short[0][0][0].cpu(), top[40:41])
    # sample_from_database(similar_to=...): the nearest item meeting the constraints, cut to the duration
    (s_top, s_bottom), s_attrs = inpainting.sample_from_database(None, encoders, 3, {}, similar_to=(long_top[..., 2:6], long_bottom[..., 4:12]),
                                                                 index=index)
    assert torch.equal(s_top.cpu(), top[40:41, :, :3]) and torch.equal(s_bottom.cpu(), bottom[40:41, :, :6]) and s_attrs["pitch"] == 64
    (s_top, _), s_attrs = inpainting.sample_from_database(None, encoders, 4, {"instrument_family_str": "fam3"},
                                                          similar_to=(q_top.unsqueeze(0), q_bottom.unsqueeze(0)), index=index)
    assert torch.equal(s_top.cpu(), top[300:301]) and s_attrs["instrument_family_str"] == "fam3"
    # the route: POST ...&nearest=1 with the sound in the body; without the new arguments it answers as before
    database = [(top[i], bottom[i], {"pitch": attrs["pitch"][i:i + 1], "instrument_family_str": attrs["instrument_family_str"][i:i + 1]})
                for i in range(N)]
    app = flask_server.create_app(vq, top_prior, bottom_prior, encoders, dev, seed=0, codes_dataset=database, codes_index=index)
    c = app.test_client()
    body = json.dumps({"top_code": top[40].tolist(), "bottom_code": bottom[40].tolist()})
    r = c.post("/sample-from-dataset?duration_top=4&nearest=1", data=body)
    assert r.status_code == 200
    assert r.get_json()["top_code"] == top[40].tolist() and r.get_json()["bottom_code"] == bottom[40].tolist()
    assert r.get_json()["top_conditioning"]["pitch"][0][0] == 64
    r = c.post("/sample-from-dataset?duration_top=4&nearest=1&instrument_family_str=fam3", data=body)
    assert r.status_code == 200 and r.get_json()["top_code"] == top[300].tolist()
    assert c.post("/sample-from-dataset?duration_top=4&nearest=1&pitch=1000", data=body).status_code == 404
    r = c.get("/sample-from-dataset?duration_top=4&pitch=64&instrument_family_str=fam7")
    assert r.status_code == 200 and r.get_json()["top_code"] == top[40].tolist()
    r = c.post("/sample-from-dataset?duration_top=4&pitch=64&instrument_family_str=fam7", data=body)      # no nearest=1: as before
    assert r.status_code == 200 and r.get_json()["top_code"] == top[40].tolist()
    no_index = flask_server.create_app(vq, top_prior, bottom_prior, encoders, dev, seed=0, codes_dataset=database)
    assert no_index.test_client().post("/sample-from-dataset?duration_top=4&nearest=1", data=body).status_code == 501
