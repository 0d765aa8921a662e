"""Host-side checks of the code-database search by encoder vectors (csrc/code_search.hip, csrc/code_shift_search.hip,
utils/datasets/code_index.py): the written specification (tests/code_soft_search_spec.py) against a
brute-force triple loop, its four contracts inside its own fp32 emulation, the lower bound by per-cell row minima, the
retrieval experiment that motivates the feature, mutants of the specification, the C-ABI's refusals before any launch, and
what `CodeIndex` validates without a device.  No GPU needed."""
import numpy as np
import pytest
import torch

import code_search_spec as S
import code_shift_search_spec as SH
import code_soft_search_spec as R

FAKE = R.FAKE


def _case(N, C, K, Q, seed, integer=True, weights="01"):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, K, (N, C)).astype(np.uint16)
    codes[0, 0] = K - 1
    if integer:
        rows = rng.integers(0, 256, (Q, C, K)).astype(np.float32)
    else:
        rows = R.rows64(rng.standard_normal((Q * C, 8)).astype(np.float32),
                        rng.standard_normal((K, 8)).astype(np.float32)).astype(np.float32).reshape(Q, C, K)
    if weights == "01":
        w = (rng.random((Q, C)) < 0.7).astype(np.float32)
    elif weights == "uniform":
        w = (2.0 * rng.random((Q, C))).astype(np.float32)
    else:
        w = None
    return codes, rows, w


def test_spec_against_a_brute_force_triple_loop():
    rng = np.random.default_rng(0)
    E = rng.standard_normal((7, 3)).astype(np.float32)
    z = rng.standard_normal((5, 3)).astype(np.float32)
    rows = R.rows64(z, E)
    for c in range(5):
        for k in range(7):
            want = 0.0
            for d in range(3):
                want += (float(z[c, d]) - float(E[k, d])) ** 2
            assert rows[c, k] == pytest.approx(want, rel=1e-15, abs=0)
    codes, rows, w = _case(5, 11, 6, 2, 1)
    codes[3, 4] = 9                                                   # a stored code >= K: clamped to K - 1
    got, mag = R.search64(codes, rows, w)
    exact = R.search_int(codes, rows, w)
    for j in range(2):
        for n in range(5):
            want = 0.0
            for c in range(11):
                want += float(w[j, c]) * float(rows[j, c, min(int(codes[n, c]), 5)])
            assert got[j, n] == want == exact[j, n] == mag[j, n]
    none, _ = R.search64(codes, rows, None)                           # null weights: 1 on every cell
    assert np.array_equal(none, R.search64(codes, rows, np.ones((2, 11), np.float32))[0])
    # the shifted form is the aligned one on cropped maps, cell c = f * W + t
    maps = rng.integers(0, 6, (4, 2, 7)).astype(np.uint16)
    wrows = rng.integers(0, 256, (1, 2 * 3, 6)).astype(np.float32)
    ww = (rng.random((1, 2, 3)) < 0.7).astype(np.float32)
    got = R.shift_search_int(maps, wrows, ww, 3, 1, 2, 2)
    for s, o in enumerate((1, 3)):
        for n in range(4):
            want = sum(int(ww[0, f, t]) * int(wrows[0, f * 3 + t, maps[n, f, t + o]]) for f in range(2) for t in range(3))
            assert got[0, s, n] == want


def test_the_four_contracts_inside_the_fp32_emulation():
    rng = np.random.default_rng(2)
    K, D = 40, 64
    E = rng.standard_normal((K, D)).astype(np.float32)
    T32 = R.rows_emulate_f32(E, E)                                    # the table kernel's arithmetic
    T64 = S.table64(E)
    assert (np.abs(T32 - T64) <= S.table_bound(T64, D)).all() and (np.diag(T32) == 0).all()
    # contract 1: vectors copied from the codebook give table rows, bit for bit; other vectors stay inside the bound
    picks = rng.integers(0, K, 30)
    z = rng.standard_normal((60, D)).astype(np.float32)
    z[:30] = E[picks]
    rows = R.rows_emulate_f32(z, E)
    assert np.array_equal(rows[:30].view(np.uint32), T32[picks].view(np.uint32))
    r64 = R.rows64(z, E)
    err = np.abs(rows - r64)
    assert (err <= R.rows_bound(r64, D)).all() and err.max() > 0
    # contract 2: gathered table rows, mask-token cells under weight 0 in both calls
    N, C, Q = 50, 600, 2
    codes = rng.integers(0, K, (N, C)).astype(np.uint16)
    query = rng.integers(0, K, (Q, C)).astype(np.uint16)
    query[rng.random((Q, C)) < 0.15] = K
    w = R.mask_token_weights(query, (2.0 * rng.random((Q, C))).astype(np.float32), K)
    hard = S.emulate_f32(codes, query, w, T32)
    soft = R.emulate_f32(codes, R.gather_rows(T32, query), w)
    assert np.array_equal(hard.view(np.uint32), soft.view(np.uint32))
    want, mag = R.search64(codes, R.gather_rows(T32, query), w)
    assert (np.abs(soft - want) <= R.search_bound(mag, C)).all()
    # contracts 3 and 4: the shifted search with gathered rows, and at W == T
    F, Tn, W = 4, 80, 72                                              # F * W = 288: two runs
    maps = rng.integers(0, K, (N, F, Tn)).astype(np.uint16)
    wq = rng.integers(0, K, (Q, F, W)).astype(np.uint16)
    ww = (2.0 * rng.random((Q, F, W))).astype(np.float32)
    hard = SH.emulate(maps, wq, ww, T32, 2, 3, 3)
    soft = R.shift_emulate(maps, R.gather_rows(T32, wq.reshape(Q, -1)), ww, W, 2, 3, 3)
    assert np.array_equal(hard.view(np.uint32), soft.view(np.uint32))
    full = R.gather_rows(T32, rng.integers(0, K, (Q, F * Tn)))
    wf = (2.0 * rng.random((Q, F, Tn))).astype(np.float32)
    at_T = R.shift_emulate(maps, full, wf, Tn, 0, 1, 1)
    aligned = R.emulate_f32(maps.reshape(N, -1), full, wf.reshape(Q, -1))
    assert np.array_equal(at_T[:, 0].view(np.uint32), aligned.view(np.uint32))


def test_lower_bound_by_row_minima():
    """dist >= sum_c w_c min_k R[c][k], with equality exactly for the item whose codes are the per-cell minima: that item
    ranks first.  Integer rows: every sum is exact, in the int64 form and in the fp32 emulation."""
    codes, rows, w = _case(200, 300, 64, 2, 3)
    for j in range(2):
        rows[j, np.arange(300), np.random.default_rng(j).integers(0, 64, 300)] = -1.0       # a unique minimum per cell
    best = rows.argmin(-1)                                            # [Q, C]
    codes[17], codes[101] = best[0], best[1]
    dist = R.search_int(codes, rows, w)
    lower = (w.astype(np.int64) * rows.min(-1).astype(np.int64)).sum(1)
    assert (dist >= lower[:, None]).all()
    assert dist[0, 17] == lower[0] and dist[1, 101] == lower[1]
    assert (np.delete(dist[0], 17) > lower[0]).all() and (np.delete(dist[1], 101) > lower[1]).all()
    assert dist.argmin(1).tolist() == [17, 101]
    assert np.array_equal(R.emulate_f32(codes, rows, w).astype(np.int64), dist)
    # and in floating point: the lower bound holds in float64 for real rows
    codes, rows, w = _case(100, 64, 32, 1, 4, integer=False, weights="uniform")
    dist, _ = R.search64(codes, rows, w)
    assert (dist >= (w.astype(np.float64) * rows.min(-1).astype(np.float64)).sum(1)[:, None] * (1 - 1e-12)).all()


def test_vector_queries_find_a_noisy_source_more_often_than_code_queries():
    """The experiment of DESIGN.md section 6c.2 in float64: K = 32 codes of D = 16 dimensions, N = 2000 random items of
    C = 8 cells, 400 trials; the query is a stored item's vectors plus Gaussian noise of sigma 2.0.  Snapping the query to
    codes first (the hard search) throws its quantisation error away; the vector query ranks its source strictly first
    in at least 40 more trials -- a third of the margin of 126 first observed (251 against 377; this file's order of
    draws gives 258 against 374)."""
    rng = np.random.default_rng(5)
    K, D, N, C, trials, sigma = 32, 16, 2000, 8, 400, 2.0
    E = rng.standard_normal((K, D)).astype(np.float32)
    codes = rng.integers(0, K, (N, C)).astype(np.uint16)
    T = S.table64(E)
    by_code = by_vector = 0
    for _ in range(trials):
        n = int(rng.integers(0, N))
        z = (E[codes[n]] + sigma * rng.standard_normal((C, D))).astype(np.float32)
        rows = R.rows64(z, E)
        soft, _ = R.search64(codes, rows[None].astype(np.float32), None)
        snapped = rows.argmin(1)[None]
        hard, _ = S.search64(codes, snapped, None, T.astype(np.float32))
        by_vector += bool(soft[0, n] < np.delete(soft[0], n).min())
        by_code += bool(hard[0, n] < np.delete(hard[0], n).min())
    print(f"source strictly first in {trials} trials: code query {by_code}, vector query {by_vector}")
    assert by_vector - by_code >= 40


def test_mutants_of_the_specification_violate_it():
    """What the GPU cases would catch: each mutant differs from the exact result on the exact cases' kind of input."""
    codes, rows, w = _case(50, 300, 64, 2, 5)
    want = R.search_int(codes, rows, w)
    # a swapped row index: cell c reads the row of cell c + 1
    assert (R.search_int(codes, np.roll(rows, 1, axis=1), w) != want).any()
    # the two queries' rows swapped
    assert (R.search_int(codes, rows[::-1], w) != want).any()
    # a weight applied after the sum instead of per cell (here: the mean weight times the unweighted sum)
    after = R.search_int(codes, rows, None) * w.mean(1)[:, None]
    assert (after != want).any()
    codes, rows, w = _case(50, 300, 64, 1, 6, integer=False, weights="uniform")
    ref, mag = R.search64(codes, rows, w)
    after = R.search64(codes, rows, None)[0] * float(w.mean())
    assert (np.abs(after - ref) > R.search_bound(mag, 300)).any()
    # a zero weight that lets NaN through: the spec answers a finite number, the mutant's 0 * NaN poisons the sum
    w[0, 17] = 0
    poisoned = rows.copy()
    poisoned[0, 17, :] = np.nan
    poisoned[0, 18, :] = np.inf
    w[0, 18] = 0
    clean, _ = R.search64(codes, poisoned, w)
    assert np.isfinite(clean).all() and np.array_equal(clean, R.search64(codes, rows, w)[0])
    assert np.isfinite(R.emulate_f32(codes, poisoned, w)).all()
    with np.errstate(invalid="ignore"):
        mutant = (poisoned[0][np.arange(300)[None, :], codes.astype(np.int64)].astype(np.float64) * w[0][None, :]).sum(1)
    assert np.isnan(mutant).all()


def test_cabi_refusals_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    err = lib.isi_last_error
    # the rows builder
    ok = dict(z=FAKE, z_stride=64, codebook=FAKE, rows=FAKE, cells=4096, K=512, D=64)

    def build(**kw):
        a = dict(ok, **kw)
        return lib.isi_code_query_rows_f32(a["z"], a["z_stride"], a["codebook"], a["rows"], a["cells"], a["K"], a["D"], None)
    for name in ("z", "codebook", "rows"):
        assert build(**{name: None}) == -1 and name.encode() in err() and b"null" in err()
        assert build(**{name: FAKE + 2}) == -1 and name.encode() in err() and b"aligned" in err()
    for name in ("cells", "K", "D"):
        for bad in (0, -1):
            assert build(**{name: bad}) == -1 and (name.encode() + b" must be positive") in err()
    assert build(z_stride=63) == -1 and b"z_stride" in err()
    assert build(z_stride=0) == -1 and build(z_stride=-5) == -1
    assert build(K=65536) == -4 and b"K beyond 65535" in err()
    assert build(cells=1 << 30) == -4 and b"cells * K" in err()      # 2^30 * 512 = 2^39
    # the aligned rows search
    ok = dict(codes=FAKE, rows=FAKE, weights=FAKE, allowed=FAKE, dist=FAKE, N=1000, C=1024, K=512, Q=2, accumulate=0,
              workspace=FAKE, workspace_bytes=1 << 30)

    def search(**kw):
        a = dict(ok, **kw)
        return lib.isi_code_search_rows_f32(a["codes"], a["rows"], a["weights"], a["allowed"], a["dist"], a["N"], a["C"],
                                            a["K"], a["Q"], a["accumulate"], a["workspace"], a["workspace_bytes"], None)
    for name in ("codes", "rows", "dist", "workspace"):
        assert search(**{name: None}) == -1
        assert name.encode() in err() and b"null" in err() and b"code_search_rows" in err()
    for name in ("N", "C", "K"):
        for bad in (0, -1):
            assert search(**{name: bad}) == -1 and (name.encode() + b" must be positive") in err()
    for bad in (0, -1, 65):
        assert search(Q=bad) == -1 and b"Q must lie in 1..64" in err()
    assert search(accumulate=2) == -1 and b"accumulate" in err()
    assert search(codes=FAKE + 1) == -1 and b"codes" in err()
    for name in ("weights", "rows", "dist", "workspace"):
        assert search(**{name: FAKE + 2}) == -1 and name.encode() in err()
    assert search(K=16385) == -4 and b"K beyond 16384" in err()
    assert search(K=65536) == -4 and b"K beyond 65535" in err()
    assert search(C=256 * 65535 + 1) == -4 and b"C beyond" in err()
    assert search(N=1 << 38, Q=2) == -4 and b"Q * N" in err()
    assert search(N=(1 << 31) * 512) == -4 and b"workgroups" in err()
    need = lib.isi_code_search_workspace_bytes(1000, 1024, 512, 2)
    assert search(workspace_bytes=need - 1) == -3 and b"workspace_bytes" in err()
    assert search(workspace_bytes=0) == -3
    # the shifted rows search
    ok = dict(codes=FAKE, rows=FAKE, weights=FAKE, dist=FAKE, N=1000, F=32, T=64, W=16, shift0=0, step=1, S=49, K=512, Q=2,
              accumulate=0, workspace=FAKE, workspace_bytes=1 << 30)

    def shifted(**kw):
        a = dict(ok, **kw)
        return lib.isi_code_shift_search_rows_f32(a["codes"], a["rows"], a["weights"], a["dist"], a["N"], a["F"], a["T"],
                                                  a["W"], a["shift0"], a["step"], a["S"], a["K"], a["Q"], a["accumulate"],
                                                  a["workspace"], a["workspace_bytes"], None)
    for name in ("codes", "rows", "dist", "workspace"):
        assert shifted(**{name: None}) == -1
        assert name.encode() in err() and b"null" in err() and b"code_shift_search_rows" in err()
    for name in ("N", "F", "T", "W", "S", "K", "step"):
        for bad in (0, -1):
            assert shifted(**{name: bad}) == -1 and (name.encode() + b" must be positive") in err()
    assert shifted(shift0=-1) == -1 and b"shift0" in err()
    assert shifted(W=65) == -1 and b"W must not exceed T" in err()
    assert shifted(S=50) == -1 and b"last offset" in err()            # 0 + 49 * 1 + 16 > 64
    assert shifted(shift0=8, S=42) == -1 and shifted(step=2, S=26) == -1
    for bad in (0, -1, 65):
        assert shifted(Q=bad) == -1 and b"Q must lie in 1..64" in err()
    assert shifted(accumulate=2) == -1 and b"accumulate" in err()
    assert shifted(codes=FAKE + 1) == -1 and b"codes" in err()
    for name in ("weights", "rows", "dist", "workspace"):
        assert shifted(**{name: FAKE + 2}) == -1 and name.encode() in err()
    assert shifted(K=16385) == -4 and b"K beyond 16384" in err()
    assert shifted(K=65536) == -4 and b"K beyond 65535" in err()
    assert shifted(F=1 << 20, T=1 << 11, W=17, S=1) == -4 and b"F * W" in err()
    assert shifted(F=1 << 15, T=1 << 16, W=16, S=1) == -4 and b"F * T" in err()
    assert shifted(N=1 << 33, Q=2, S=49) == -4 and b"Q * S * N" in err()
    need = lib.isi_code_shift_search_workspace_bytes(1000, 32, 64, 16, 49, 512, 2)
    assert need == 2 * 2 * 49 * 1000 * 4
    assert shifted(workspace_bytes=need - 1) == -3 and b"workspace_bytes" in err()
    small = lib.isi_code_shift_search_workspace_bytes(1000, 8, 64, 16, 49, 512, 2)
    assert small == 16 and shifted(F=8, workspace_bytes=15) == -3


def _vqvae(n_embed=32):
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    return VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
                 num_embeddings=n_embed, resolution_factors={"bottom": 4, "top": 2})


def test_code_index_validation_needs_no_device():
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.datasets import code_index
    from interactive_spectrogram_inpainting.utils.datasets.code_index import CodeIndex
    import inpainting
    assert 0 < code_index.ROWS_BUDGET_BYTES <= 1 << 30
    vq = _vqvae()
    g = torch.Generator().manual_seed(0)
    top, bottom = torch.randint(0, 32, (20, 8, 4), generator=g), torch.randint(0, 32, (20, 16, 8), generator=g)
    index = CodeIndex.from_arrays(top, bottom, {"pitch": torch.arange(20)}, vq, "cpu")
    z_t, z_b = torch.randn(8, 4, 16, generator=g), torch.randn(16, 8, 16, generator=g)
    r_t = torch.rand(1, 8, 4, 32, generator=g)
    for search in (index.search_soft, index.search_shifted_soft, index.distances_soft, index.distances_shifted_soft):
        with pytest.raises(ValueError):
            search()
        # two forms for one layer
        with pytest.raises(ValueError, match="one of top_code, top_vectors and top_rows"):
            search(top[0], top_vectors=z_t)
        with pytest.raises(ValueError, match="one of bottom_code"):
            search(top_vectors=z_t, bottom_vectors=z_b, bottom_rows=torch.rand(1, 16, 8, 32))
        # wrong D, wrong K, wrong cells, wrong type
        with pytest.raises(ValueError, match="top_vectors"):
            search(top_vectors=torch.randn(8, 4, 15))
        with pytest.raises(ValueError, match="top_rows"):
            search(top_rows=torch.rand(1, 8, 4, 33))
        with pytest.raises(ValueError, match="bottom_vectors"):
            search(bottom_vectors=torch.randn(15, 8, 16))
        with pytest.raises(ValueError, match="top_vectors"):
            search(top_vectors=torch.zeros(8, 4, 16, dtype=torch.int64))
        # Q > 64, and layers that disagree on Q
        with pytest.raises(ValueError, match="65 queries"):
            search(top_vectors=torch.randn(65, 8, 4, 16))
        with pytest.raises(ValueError, match="65 queries"):
            search(top_rows=torch.rand(65, 8, 4, 32))
        with pytest.raises(ValueError, match="different numbers of queries"):
            search(top_vectors=torch.randn(3, 8, 4, 16), bottom_code=bottom[:2])
        with pytest.raises(ValueError, match="mask_top"):
            search(top_vectors=z_t, mask_top=torch.zeros(8, 3, dtype=torch.bool))
        with pytest.raises(ValueError, match="layer_weights"):
            search(top_vectors=z_t, layer_weights=(-1.0, 1.0))
        # then: no CPU path, in any form or mixture of forms
        with pytest.raises(_hip.HipLibraryError):
            search(top_vectors=z_t, bottom_vectors=z_b)
        with pytest.raises(_hip.HipLibraryError):
            search(top_rows=r_t)
        with pytest.raises(_hip.HipLibraryError):
            search(top_vectors=z_t, bottom_code=bottom[0])
    with pytest.raises(ValueError):
        index.search_soft(top_vectors=z_t, k=0)
    with pytest.raises(ValueError):
        index.search_soft(top_vectors=z_t[:, :3])                      # the aligned search takes whole maps only
    with pytest.raises(ValueError, match="bottom window"):
        index.search_shifted_soft(top_vectors=z_t[:, :2], bottom_vectors=z_b[:, :5])
    with pytest.raises(ValueError, match="shift_range"):
        index.search_shifted_soft(top_vectors=z_t[:, :2], shift_range=(3, 9))
    with pytest.raises(LookupError):                                   # nobody admitted: said before any upload or launch
        index.search_soft(top_vectors=z_t, bottom_vectors=z_b, attribute_constraints={"pitch": 1000})
    with pytest.raises(LookupError):
        index.search_shifted_soft(top_vectors=z_t[:, :2], bottom_vectors=z_b[:, :4], attribute_constraints={"pitch": 1000})
    no_bottom = CodeIndex.from_arrays(top, None, {}, vq, "cpu")
    with pytest.raises(ValueError, match="holds no bottom maps"):
        no_bottom.search_soft(top_vectors=z_t, bottom_vectors=z_b)
    with pytest.raises(_hip.HipLibraryError):
        vq.quantize_t.distance_rows(z_t)
    with pytest.raises(_hip.HipLibraryError):
        vq.eval().encode_vectors(torch.randn(1, 2, 32, 64))
    with pytest.raises(RuntimeError, match="eval-mode"):
        vq.train().encode_vectors(torch.randn(1, 2, 32, 64))
    for name in ("similar_sounds_to_spectrogram", "similar_fragments_to_spectrogram", "similar_to_mixture"):
        assert callable(getattr(inpainting, name))
