"""Host-side checks of the time-warped code search (csrc/code_warp_search.hip, utils/datasets/code_index.py; DESIGN.md
section 6c.3): the written specification (tests/code_warp_search_spec.py) against a brute-force enumeration of every
admissible path, the derived bound for its own fp32 emulation on every shape the GPU tests use, planted faults that the
comparison must reject on those inputs, the closed band against the shifted search's specification, the C-ABI's refusals
before any launch, `paste_warped`, and what `CodeIndex.search_warped` validates without a device.  No GPU needed.

GEOMETRIES, `parts_of` and `reference` are shared with tests/test_code_warp_search_gpu.py: the references are computed
once and nobody changes them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import code_search_spec as S
import code_shift_search_spec as SH
import code_warp_search_spec as WS

FAKE = S.FAKE

#             name                N    T   W   lo  hi  Q  parts (F, r, K)
GEOMETRIES = [("smallest",        1,   1,  1,  0,  0,  1, ((1, 1, 2),)),
              ("ragged-clipped",  300, 12, 7,  -2, 3,  2, ((3, 1, 7),)),        # two workgroups, band clipped at both item ends
              ("w-beyond-t",      70,  9,  12, -5, 0,  1, ((5, 1, 11),)),       # W > T
              ("widest-band",     130, 80, 10, 0,  63, 1, ((2, 1, 33),)),       # 64 drifts
              ("band-of-23",      100, 40, 9,  -10, 12, 1, ((2, 1, 19),)),      # the 32-wide register band
              ("two-layers",      260, 10, 8,  -1, 2,  2, ((3, 1, 7), (4, 2, 300))),
              ("narrow-group",    50,  12, 9,  -2, 2,  1, ((4, 1, 4100),)),     # a group of 8 columns does not fit the stage
              ("cell-at-a-time",  40,  6,  3,  -1, 1,  1, ((2, 1, 5), (1, 2, 8200))),   # not even one row of one column fits
              ("real",            600, 64, 64, -8, 8,  1, ((16, 1, 512), (32, 2, 512)))]
IDS = [g[0] for g in GEOMETRIES]


def geometry(name):
    return next(g for g in GEOMETRIES if g[0] == name)


@functools.lru_cache(maxsize=None)
def parts_of(name, integer):
    """The shared inputs of one geometry: integer rows in [0, 255] with 0/1 weights, or float rows >= 0 with weights in
    [0, 2); in both, every cell of weight 0 has a NaN or an inf row, and one stored code lies beyond K - 1."""
    _, N, T, W, lo, hi, Q, layout = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) + (1000 if integer else 0))
    parts = []
    for F, r, K in layout:
        codes = rng.integers(0, K, (N, F, T * r)).astype(np.uint16)
        codes[N - 1, F - 1, T * r - 1] = K - 1
        codes[0, 0, 0] = K + 3                                         # clamped to K - 1
        if integer:
            rows = rng.integers(0, 256, (Q, F * W * r, K), dtype=np.uint8).astype(np.float32)
            w = (rng.random((Q, F, W * r)) < 0.7).astype(np.float32)
        else:
            rows = (rng.standard_normal((Q, F * W * r, K), dtype=np.float32) ** 2 * 16).astype(np.float32)
            w = (2.0 * rng.random((Q, F, W * r))).astype(np.float32)
            w[rng.random((Q, F, W * r)) < 0.1] = 0
        w[0, 0, 0] = 1.0
        dead = np.argwhere(w.reshape(Q, -1) == 0)
        rows[dead[::2, 0], dead[::2, 1], :] = np.nan
        rows[dead[1::2, 0], dead[1::2, 1], :] = np.inf
        parts.append(WS.Part(codes, rows, w, r))
    return tuple(parts)


@functools.lru_cache(maxsize=None)
def reference(name, integer):
    """(dist, end, path) of the shared inputs: the int64 specification, or the fp32 emulation."""
    _, N, T, W, lo, hi, Q, _ = geometry(name)
    parts = list(parts_of(name, integer))
    return WS.search_int(parts, lo, hi) if integer else WS.emulate(parts, lo, hi)


@functools.lru_cache(maxsize=None)
def reference64(name):
    _, N, T, W, lo, hi, Q, _ = geometry(name)
    return WS.search64(list(parts_of(name, False)), lo, hi)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("W,T,lo,hi", [(1, 1, 0, 0), (3, 3, 0, 0), (4, 6, -1, 2), (5, 6, -2, 1), (5, 4, -3, 0), (2, 6, 0, 4),
                                       (5, 5, -4, 4), (4, 6, 2, 2)])
def test_recurrence_equals_brute_force_over_every_path(W, T, lo, hi):
    """fp32 bit for bit and int64 exactly, one and two parts; the path the specification returns is admissible and its
    left-to-right sum IS the distance."""
    rng = np.random.default_rng(W * 100 + T * 10 + hi - lo)
    N, Q = 6, 2
    assert WS.has_path(W, T, lo, hi)
    for layout in (((2, 1, 5),), ((2, 1, 5), (3, 2, 4))):
        for integer in (False, True):
            parts = []
            for F, r, K in layout:
                codes = rng.integers(0, K, (N, F, T * r)).astype(np.uint16)
                rows = rng.integers(0, 4, (Q, F * W * r, K)).astype(np.float32) if integer \
                    else rng.random((Q, F * W * r, K)).astype(np.float32)
                w = (rng.random((Q, F, W * r)) < 0.8).astype(np.float32) * (1 if integer else np.float32(1.7))
                parts.append(WS.Part(codes, rows, w, r))
            dtype = np.int64 if integer else np.float32
            dist, end, path = WS.search_int(parts, lo, hi) if integer else WS.emulate(parts, lo, hi)
            for j in range(Q):
                cost = WS.column_cost(parts, j, dtype)
                for n in range(N):
                    want = WS.brute_force(cost[n], lo, hi)
                    assert want is not None and want.dtype == dtype
                    assert dist[j, n] == want and (integer or _bits(dist[j, n]) == _bits(want))
                    assert WS.path_admissible(path[j, n], T, lo, hi) and path[j, n, -1] == end[j, n]
                    total = cost[n, 0, path[j, n, 0]]
                    for i in range(1, W):
                        total = cost[n, i, path[j, n, i]] + total
                    assert total == dist[j, n]


def test_no_path_and_allowed():
    rng = np.random.default_rng(3)
    part = WS.Part(rng.integers(0, 4, (5, 2, 6)), rng.random((1, 2 * 3, 4)).astype(np.float32))
    assert not WS.has_path(3, 6, 6, 7) and not WS.has_path(3, 6, -5, -3) and WS.has_path(3, 6, -2, 3)
    dist, end, path = WS.emulate([part], 6, 7)
    assert np.isposinf(dist).all() and (end == -1).all() and (path == -1).all()
    allowed = np.array([1, 0, 1, 1, 0], np.uint8)
    dist, end, path = WS.emulate([part], -2, 3, allowed)
    assert np.isposinf(dist[0, [1, 4]]).all() and (end[0, [1, 4]] == -1).all() and (path[0, [1, 4]] == -1).all()
    assert np.isfinite(dist[0, [0, 2, 3]]).all() and (end[0, [0, 2, 3]] >= 0).all()


@pytest.mark.parametrize("name", IDS)
def test_emulation_inside_the_derived_bound_on_every_gpu_shape(name):
    """The inputs the kernel is held to the bound on satisfy it in the emulation; the integer inputs stay exact in fp32."""
    _, N, T, W, lo, hi, Q, _ = geometry(name)
    parts = list(parts_of(name, False))
    got, want = reference(name, False)[0], reference64(name)
    assert got.dtype == np.float32 and np.isfinite(want).all() and (want >= 0).all()
    err, bound = np.abs(got.astype(np.float64) - want), WS.bound(want, parts)
    print(f"warp emulation {name}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}, "
          f"bound = {WS.grid(parts)[4] + W + 2} u")
    assert (err <= bound).all()
    exact = reference(name, True)[0]
    assert exact.max() + 1000 < 2 ** 24 and exact.min() >= 0
    assert np.array_equal(WS.emulate(list(parts_of(name, True)), lo, hi)[0].astype(np.int64), exact)


def _padded(parts, pad):
    """The items continued on both sides by `pad` columns of what lies beside them in memory (their own row, wrapped): a
    band that is not clipped at the item's ends walks into them."""
    return [WS.Part(np.pad(p.codes, ((0, 0), (0, 0), (pad * p.r, pad * p.r)), mode="wrap"), p.rows, p.weights, p.r) for p in parts]


@pytest.mark.parametrize("name", ["ragged-clipped", "two-layers"])
def test_planted_faults_are_rejected_on_the_test_inputs(name):
    _, N, T, W, lo, hi, Q, _ = geometry(name)
    for integer in (True, False):
        parts = list(parts_of(name, integer))
        run = WS.search_int if integer else WS.emulate
        same = (lambda a, b: np.array_equal(a, b)) if integer else (lambda a, b: np.array_equal(_bits(a), _bits(b)))
        dist, end, path = reference(name, integer)
        assert not same(run(parts, lo, hi, steps=(1, 0))[0], dist), "no skip step"
        assert not same(run(parts, lo, hi, steps=(1, 2))[0], dist), "no hold"
        pad = max(abs(lo), abs(hi)) + W
        wide = _padded(parts, pad)
        got = (WS.search_int(wide, lo + pad, hi + pad) if integer else WS.emulate(wide, lo + pad, hi + pad))[0]
        assert not same(got, dist) and (got <= dist).all(), "band not clipped at the item's ends"
        other = run(parts, lo, hi, steps=(0, 1, 2))                                    # the wrong tie rule: paths only
        assert same(other[0], dist) and (not integer or not np.array_equal(other[2], path))    # (floats hardly ever tie)
    if name == "two-layers":
        parts = list(parts_of(name, False))
        assert not np.array_equal(_bits(WS.emulate(parts[::-1], lo, hi)[0]), _bits(reference(name, False)[0])), \
            "parts summed in the other order"
        assert np.array_equal(WS.search_int(list(parts_of(name, True))[::-1], lo, hi)[0], reference(name, True)[0])


def test_closed_band_is_the_shifted_search_and_wider_bands_never_increase():
    rng = np.random.default_rng(17)
    N, F, T, W, K, Q = 40, 3, 12, 7, 9, 2
    codes = rng.integers(0, K, (N, F, T)).astype(np.uint16)
    query = rng.integers(0, K + 1, (Q, F, W)).astype(np.uint16)                        # K: the mask token
    table = rng.integers(0, 256, (K, K)).astype(np.float32)
    w = (rng.random((Q, F, W)) < 0.7).astype(np.float32)
    rows = table[np.where(query < K, query, 0)].reshape(Q, F * W, K)
    part = WS.Part(codes, rows, np.where(query >= K, 0, w).astype(np.float32))
    want = SH.search_int(codes, query, w, table, 0, 1, T - W + 1)                      # [Q, S, N]
    for o in range(T - W + 1):
        dist, end, path = WS.search_int([part], o, o)
        assert np.array_equal(dist, want[:, o]) and (end == o + W - 1).all() and (path == o + np.arange(W)).all()
    floats = WS.Part(codes, (rng.standard_normal((Q, F * W, K), dtype=np.float32) ** 2).astype(np.float32), w)
    bands = [(2, 2), (1, 3), (-1, 4), (-6, 5)]
    dists = [WS.emulate([floats], lo, hi)[0] for lo, hi in bands]
    for narrow, wide in zip(dists, dists[1:]):
        assert (wide <= narrow).all()
    assert (dists[-1] < dists[0]).any()


# -------------------------------------------------------------------------------------------------------- the C-ABI
def check_cabi_refusals(lib):
    """Every refusal of isi_code_warp_search_f32 and isi_code_warp_path_f32, before any launch (the pointers are never
    dereferenced).  Shared with the GPU tests."""
    from interactive_spectrogram_inpainting import _hip
    err = lib.isi_last_error
    ok = dict(n_parts=2, allowed=FAKE, dist=FAKE, end=FAKE, N=1000, T=64, W=64, lo=-8, hi=8, Q=2, items=FAKE, M=8, path=FAKE,
              workspace=FAKE, workspace_bytes=1 << 30)
    ok_parts = [dict(codes=FAKE, rows=FAKE, weights=FAKE, F=16, r=1, K=512), dict(codes=FAKE, rows=FAKE, weights=None, F=32, r=2, K=512)]

    def call(which, part=None, parts_null=False, **kw):
        a = dict(ok, **{k: v for k, v in kw.items() if k in ok})
        descr = [dict(p) for p in ok_parts]
        if part is not None:
            descr[part].update({k: v for k, v in kw.items() if k not in ok})
        else:
            for p in descr:
                p.update({k: v for k, v in kw.items() if k not in ok})
        array = (_hip.isi_warp_part * 2)()
        for p, d in zip(array, descr):
            p.codes, p.rows, p.weights, p.F, p.r, p.K = d["codes"], d["rows"], d["weights"], d["F"], d["r"], d["K"]
        handle = None if parts_null else array
        if which == "search":
            return lib.isi_code_warp_search_f32(handle, a["n_parts"], a["allowed"], a["dist"], a["end"], a["N"], a["T"], a["W"],
                                                a["lo"], a["hi"], a["Q"], None)
        return lib.isi_code_warp_path_f32(handle, a["n_parts"], a["items"], a["M"], a["path"], a["dist"], a["workspace"],
                                          a["workspace_bytes"], a["N"], a["T"], a["W"], a["lo"], a["hi"], a["Q"], None)
    for which, fn in (("search", b"code_warp_search"), ("path", b"code_warp_path")):
        assert call(which, parts_null=True) == -1 and b"parts is a null" in err() and fn in err()
        for part in (0, 1):
            for name in ("codes", "rows"):
                assert call(which, part=part, **{name: None}) == -1 and name.encode() in err() and b"null" in err()
            assert call(which, part=part, codes=FAKE + 1) == -1 and b"codes must be aligned" in err()
            assert call(which, part=part, rows=FAKE + 2) == -1 and b"rows must be aligned" in err()
            assert call(which, part=part, weights=FAKE + 2) == -1 and b"weights must be aligned" in err()
            for name in ("F", "r", "K"):
                for bad in (0, -1):
                    assert call(which, part=part, **{name: bad}) == -1 and (name.encode() + b" must be positive") in err()
            assert call(which, part=part, K=16385) == -4 and b"K beyond 16384" in err()
            assert call(which, part=part, K=65536) == -4 and b"K beyond 65535" in err()
            assert call(which, part=part, F=1 << 26) == -4 and b"beyond 2^31" in err()
        for name in ("N", "T", "W"):
            for bad in (0, -1):
                assert call(which, **{name: bad}) == -1 and (name.encode() + b" must be positive") in err()
        for bad in (0, 3, -1):
            assert call(which, n_parts=bad) == -1 and b"n_parts must be 1 or 2" in err()
        for bad in (0, -1, 65):
            assert call(which, Q=bad) == -1 and b"Q must lie in 1..64" in err()
        assert call(which, dist=None) == -1 and b"dist is a null" in err()
        assert call(which, dist=FAKE + 2) == -1 and b"dist must be aligned" in err()
        assert call(which, lo=3, hi=2) == -1 and b"lo must not exceed hi" in err()
        assert call(which, lo=-9, hi=-1) == -1 and b"first query column" in err()       # hi < 0
        assert call(which, lo=64, hi=70) == -1 and b"first query column" in err()       # lo > T - 1
        assert call(which, lo=1, hi=5) == -1 and b"last query column" in err()          # W - 1 + lo > T - 1
        assert call(which, W=100, T=20, lo=-60, hi=0) == -1 and b"last query column" in err()
        assert call(which, T=200, lo=0, hi=64) == -4 and b"more than 64 drifts" in err()
        assert call(which, W=4097, T=5000, lo=0, hi=3) == -4 and b"W beyond 4096" in err()
    assert call("search", end=FAKE + 2) == -1 and b"end must be aligned" in err()
    assert call("search", N=1 << 38) == -4 and b"Q * N beyond 2^39" in err()
    for name in ("items", "path", "workspace"):
        assert call("path", **{name: None}) == -1 and name.encode() in err() and b"null" in err()
    assert call("path", items=FAKE + 4) == -1 and b"items must be aligned" in err()
    assert call("path", path=FAKE + 2) == -1 and b"path must be aligned" in err()
    for bad in (0, -1, 65):
        assert call("path", M=bad) == -1 and b"M must lie in 1..64" in err()
    need = lib.isi_code_warp_path_workspace_bytes(8, 64, -8, 8, 2)
    assert need == 2 * 8 * 64 * 17
    assert call("path", workspace_bytes=need - 1) == -3 and b"workspace_bytes" in err()
    assert lib.isi_code_warp_path_workspace_bytes(3, 5, 0, 0, 1) == 16                  # 15 bytes, rounded up
    for bad in ((0, 64, -8, 8, 2), (65, 64, -8, 8, 2), (8, 0, -8, 8, 2), (8, 4097, -8, 8, 2), (8, 64, 1, 0, 2), (8, 64, 0, 64, 2),
                (8, 64, -8, 8, 0), (8, 64, -8, 8, 65)):
        assert lib.isi_code_warp_path_workspace_bytes(*bad) == 0


def test_cabi_refusals_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    assert C.sizeof(_hip.isi_warp_part) == 40
    check_cabi_refusals(_hip.lib())


# ------------------------------------------------------------------------------------------------------------ Python
def test_paste_warped_is_paste_fragment_on_a_straight_path_and_follows_a_bent_one():
    import inpainting
    g = torch.Generator().manual_seed(5)
    top, bottom = torch.randint(0, 32, (1, 4, 10), generator=g), torch.randint(0, 32, (1, 8, 20), generator=g)
    item_top, item_bottom = torch.randint(0, 32, (1, 4, 12), generator=g), torch.randint(0, 32, (1, 8, 24), generator=g)
    W, start = 5, 3
    mask = torch.rand(1, 4, W, generator=g) < 0.6
    mask_b = torch.rand(1, 8, 2 * W, generator=g) < 0.6
    for shift in (0, 2, 6, 9, -2):                                    # the last two leave the item
        path = shift + torch.arange(W)
        for layer, m in (("top", mask), ("bottom", mask_b)):
            want = inpainting.paste_fragment(top, bottom, item_top, item_bottom, m, layer, start, shift)
            got = inpainting.paste_warped(top, bottom, item_top, item_bottom, m, start, path, layer=layer)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    path = torch.tensor([4, 4, 5, 7, 8])                              # hold, step, skip, step
    full = torch.ones(1, 4, W, dtype=torch.bool)
    new_top, new_bottom = inpainting.paste_warped(top, bottom, item_top, item_bottom, full, start, path)
    for i, p in enumerate(path.tolist()):
        assert torch.equal(new_top[0, :, start + i], item_top[0, :, p])
        assert torch.equal(new_bottom[0, :, 2 * (start + i):2 * (start + i) + 2], item_bottom[0, :, 2 * p:2 * p + 2])
    assert torch.equal(new_top[..., :start], top[..., :start]) and torch.equal(new_top[..., start + W:], top[..., start + W:])
    assert torch.equal(new_bottom[..., 2 * (start + W):], bottom[..., 2 * (start + W):])
    gone = inpainting.paste_warped(top, bottom, item_top, item_bottom, full, start, torch.full((W,), -1))
    assert torch.equal(gone[0], top) and torch.equal(gone[1], bottom)                  # no path: nothing is pasted
    with pytest.raises(ValueError, match="mask"):
        inpainting.paste_warped(top, bottom, item_top, item_bottom, full[..., :4], start, path)
    with pytest.raises(ValueError, match="layer"):
        inpainting.paste_warped(top, bottom, item_top, item_bottom, full, start, path, layer="middle")


def test_paste_fragment_takes_a_bottom_mask_of_odd_width():
    """A bottom-layer window need not be a whole number of top columns: 3 bottom columns on maps of time ratio 2 (a width
    `paste_warped`, whose mask spans r W columns, cannot express)."""
    import inpainting
    g = torch.Generator().manual_seed(5)
    top, bottom = torch.randint(0, 32, (1, 4, 10), generator=g), torch.randint(0, 32, (1, 8, 20), generator=g)
    item_top, item_bottom = torch.randint(0, 32, (1, 4, 12), generator=g), torch.randint(0, 32, (1, 8, 24), generator=g)
    mask = torch.rand(1, 8, 3, generator=g) < 0.6
    assert mask.any() and not mask.all()
    for start, shift in ((3, 2), (0, 0), (9, 11), (2, -1)):            # bottom columns 2 start + c from item columns 2 shift + c
        new_top, new_bottom = inpainting.paste_fragment(top, bottom, item_top, item_bottom, mask, "bottom", start, shift)
        want = bottom.clone()
        for c in range(3):
            column, source = 2 * start + c, 2 * shift + c
            if 0 <= column < 20 and 0 <= source < 24:
                want[0, :, column] = torch.where(mask[0, :, c], item_bottom[0, :, source], bottom[0, :, column])
        assert torch.equal(new_bottom, want) and torch.equal(new_top, top) and new_top is not top


def _vqvae(n_embed=32):
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    return VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
                 num_embeddings=n_embed, resolution_factors={"bottom": 4, "top": 2})


def test_search_warped_validation_needs_no_device():
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.datasets import code_index
    from interactive_spectrogram_inpainting.utils.datasets.code_index import CodeIndex
    import inpainting
    assert code_index.MAX_DRIFTS == 64 and code_index.MAX_PATH_ITEMS == 64
    vq = _vqvae()
    g = torch.Generator().manual_seed(0)
    top, bottom = torch.randint(0, 32, (20, 8, 4), generator=g), torch.randint(0, 32, (20, 16, 8), generator=g)
    index = CodeIndex.from_arrays(top, bottom, {"pitch": torch.arange(20)}, vq, "cpu")
    z_t, z_b = torch.randn(8, 4, 16, generator=g), torch.randn(16, 8, 16, generator=g)
    searches = (index.search_warped, index.distances_warped, lambda *a, **kw: index.warp_paths([0, 1], *a, **kw))
    for search in searches:
        with pytest.raises(ValueError):
            search()
        with pytest.raises(ValueError, match="one of top_code, top_vectors and top_rows"):
            search(top[0], top_vectors=z_t)
        with pytest.raises(ValueError, match="top_vectors"):
            search(top_vectors=torch.randn(8, 4, 15))
        with pytest.raises(ValueError, match="top_rows"):
            search(top_rows=torch.rand(1, 8, 4, 33))
        with pytest.raises(ValueError, match="65 queries"):
            search(top_vectors=torch.randn(65, 8, 4, 16))
        with pytest.raises(ValueError, match="different numbers of queries"):
            search(top_vectors=torch.randn(3, 8, 4, 16), bottom_code=bottom[:2])
        with pytest.raises(ValueError, match="mask_top"):
            search(top_vectors=z_t, mask_top=torch.zeros(8, 3, dtype=torch.bool))
        with pytest.raises(ValueError, match="layer_weights"):
            search(top_vectors=z_t, layer_weights=(-1.0, 1.0))
        with pytest.raises(ValueError, match="bottom window"):
            search(top_vectors=z_t[:, :2], bottom_vectors=z_b[:, :5])
        # the band
        with pytest.raises(ValueError, match="drift"):
            search(top[0], drift=(1,))
        with pytest.raises(ValueError, match="drift"):
            search(top[0], drift=None)
        with pytest.raises(ValueError, match="lo must not exceed hi"):
            search(top[0], drift=(2, 1))
        with pytest.raises(ValueError, match="at most 64"):
            search(top[0], drift=(-32, 32))
        with pytest.raises(ValueError, match="first or the last"):
            search(top[0], drift=(1, 2))                               # a whole map cannot start late
        with pytest.raises(ValueError, match="first or the last"):
            search(top[0], drift=(-3, -1))
        with pytest.raises(ValueError, match="first or the last"):
            search(top[0, :, :2], drift=(3, 5))                        # a window of 2 columns fits at offsets 0 .. 2
        # then: no CPU path, in any form
        with pytest.raises(_hip.HipLibraryError):
            search(top[0], bottom[0])
        with pytest.raises(_hip.HipLibraryError):
            search(top_vectors=z_t, bottom_code=bottom[0], drift=(0, 0))
        with pytest.raises(_hip.HipLibraryError):
            search(top[0, :, :2], drift=(0, 2))
    with pytest.raises(ValueError):
        index.search_warped(top[0], k=0)
    with pytest.raises(LookupError):                                   # nobody admitted: said before any upload or launch
        index.search_warped(top[0], bottom[0], attribute_constraints={"pitch": 1000})
    no_bottom = CodeIndex.from_arrays(top, None, {}, vq, "cpu")
    with pytest.raises(ValueError, match="holds no bottom maps"):
        no_bottom.search_warped(top[0], bottom[0])
    assert callable(inpainting.similar_sounds_warped) and callable(inpainting.paste_warped)
