"""Host-side checks of the code-database search (csrc/code_search.hip, utils/datasets/code_index.py): the written
specification (tests/code_search_spec.py) against a brute-force triple loop, the fp32 emulation of the kernel's arithmetic
inside the derived bound at C = 4096, mutants of the specification outside it (so the GPU cases have teeth), the C-ABI's
refusals before any launch, and what `CodeIndex` validates without a device.  No GPU needed."""
import numpy as np
import pytest
import torch

import code_search_spec as S

FAKE = S.FAKE


def _case(N, C, K, Q, seed, integer=True, mask_tokens=True, weights="01"):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, K, (N, C)).astype(np.uint16)
    codes[0, 0] = K - 1
    query = rng.integers(0, K, (Q, C)).astype(np.uint16)
    if mask_tokens and C > 1:
        query[rng.random((Q, C)) < 0.15] = K                          # the priors' mask token: counts nothing
    if integer:
        table = rng.integers(0, 256, (K, K)).astype(np.float32)       # asymmetric on purpose
    else:
        table = S.table64(rng.standard_normal((K, 8)).astype(np.float32)).astype(np.float32)
    if weights == "01":
        w = (rng.random((Q, C)) < 0.7).astype(np.float32)
    elif weights == "uniform":
        w = (2.0 * rng.random((Q, C))).astype(np.float32)
    else:
        w = None
    return codes, query, w, table


def test_spec_against_a_brute_force_triple_loop():
    rng = np.random.default_rng(0)
    E = rng.standard_normal((7, 3)).astype(np.float32)
    T = S.table64(E)
    for a in range(7):
        for b in range(7):
            want = 0.0
            for d in range(3):
                want += (float(E[a, d]) - float(E[b, d])) ** 2
            assert T[a, b] == pytest.approx(want, rel=1e-15, abs=0)
    assert (np.diag(T) == 0).all() and np.array_equal(T, T.T)
    codes, query, w, table = _case(5, 11, 6, 2, 1)
    got, mag = S.search64(codes, query, w, table)
    exact = S.search_int(codes, query, w, table)
    for j in range(2):
        for n in range(5):
            want = 0.0
            for c in range(11):
                if query[j, c] < 6:
                    want += float(w[j, c]) * float(table[query[j, c], codes[n, c]])
            assert got[j, n] == want == exact[j, n] == mag[j, n]
    assert (query == 6).any()
    none, _ = S.search64(codes, query, None, table)                   # null weights: 1 on every cell
    assert np.array_equal(none, S.search64(codes, query, np.ones((2, 11), np.float32), table)[0])
    assert np.array_equal(S.apply_allowed(got, np.array([1, 0, 1, 1, 0]))[:, [1, 4]], np.full((2, 2), np.inf))


def test_fp32_emulation_stays_inside_the_bound_at_4096_cells():
    codes, query, w, table = _case(64, 4096, 512, 2, 2, integer=False, weights="uniform")
    want, mag = S.search64(codes, query, w, table)
    got = S.emulate_f32(codes, query, w, table).astype(np.float64)
    err = np.abs(got - want)
    assert (err <= S.search_bound(mag, 4096)).all()
    assert err.max() > 0                                              # the bound is not vacuous: fp32 does round here
    # integer tables, 0/1 weights, sums below 2^24: the same arithmetic is exact
    codes, query, w, table = _case(64, 4096, 512, 2, 3)
    assert np.array_equal(S.emulate_f32(codes, query, w, table).astype(np.int64), S.search_int(codes, query, w, table))
    # the table's bound against its own fp32 emulation (differences and fma chain in fp32)
    E = np.random.default_rng(4).standard_normal((40, 64)).astype(np.float32)
    t32 = np.zeros((40, 40), np.float32)
    for d in range(64):
        diff = (E[:, None, d] - E[None, :, d]).astype(np.float32)
        t32 = (diff.astype(np.float64) * diff.astype(np.float64) + t32.astype(np.float64)).astype(np.float32)   # one rounding: fma
    t64 = S.table64(E)
    assert (np.abs(t32 - t64) <= S.table_bound(t64, 64)).all() and (np.diag(t32) == 0).all()


def test_mutants_of_the_specification_violate_it():
    """What the GPU cases would catch: each mutant differs from the exact result on the exact cases' kind of input."""
    codes, query, w, table = _case(50, 300, 64, 2, 5)
    want = S.search_int(codes, query, w, table)
    # one cell dropped (a live, weighted one)
    j, c = np.argwhere((query < 64) & (w > 0))[-1]
    dropped = w.copy()
    dropped[j, c] = 0
    assert (S.search_int(codes, query, dropped, table) != want).any()
    # a weight ignored
    assert (S.search_int(codes, query, None, table) != want).any()
    # a mask-token cell counted (as if it were code K - 1)
    counted = np.where(query >= 64, 63, query)
    assert (S.search_int(codes, counted, w, table) != want).any()
    # table row and column swapped, on the asymmetric table
    assert not np.array_equal(table, table.T)
    assert (S.search_int(codes, query, w, table.T.copy()) != want).any()
    # and in floating point the first mutant leaves the bound
    codes, query, w, table = _case(50, 300, 64, 1, 6, integer=False, mask_tokens=False, weights="uniform")
    ref, mag = S.search64(codes, query, w, table)
    dropped = w.copy()
    dropped[0, 17] = 0
    bad, _ = S.search64(codes, query, dropped, table)
    assert (np.abs(bad - ref) > S.search_bound(mag, 300)).any()


def test_cabi_refusals_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    # the table
    ok = dict(codebook=FAKE, table=FAKE, K=512, D=64)

    def table(**kw):
        a = dict(ok, **kw)
        return lib.isi_code_distance_table_f32(a["codebook"], a["table"], a["K"], a["D"], None)
    for name in ("codebook", "table"):
        assert table(**{name: None}) == -1 and name.encode() in lib.isi_last_error() and b"null" in lib.isi_last_error()
        assert table(**{name: FAKE + 2}) == -1 and name.encode() in lib.isi_last_error()
    assert table(K=0) == -1 and b"K" in lib.isi_last_error()
    assert table(D=0) == -1 and b"D" in lib.isi_last_error()
    assert table(K=-3) == -1 and table(D=-1) == -1
    assert table(K=65536) == -4 and b"K" in lib.isi_last_error()
    # the search
    assert lib.isi_code_search_workspace_bytes(1000, 1024, 512, 1) == 4 * 1000 * 4
    assert lib.isi_code_search_workspace_bytes(1000, 1025, 512, 3) == 5 * 3 * 1000 * 4
    assert lib.isi_code_search_workspace_bytes(305979, 4096, 512, 8) == 16 * 8 * 305979 * 4
    assert lib.isi_code_search_workspace_bytes(0, 1024, 512, 1) == 0 and lib.isi_code_search_workspace_bytes(10, 10, 10, 65) == 0
    ok = dict(codes=FAKE, query=FAKE, weights=FAKE, table=FAKE, allowed=FAKE, dist=FAKE, N=1000, C=1024, K=512, Q=2,
              accumulate=0, workspace=FAKE, workspace_bytes=1 << 30)

    def search(**kw):
        a = dict(ok, **kw)
        return lib.isi_code_search_f32(a["codes"], a["query"], a["weights"], a["table"], a["allowed"], a["dist"], a["N"],
                                       a["C"], a["K"], a["Q"], a["accumulate"], a["workspace"], a["workspace_bytes"], None)
    for name in ("codes", "query", "table", "dist", "workspace"):
        assert search(**{name: None}) == -1
        assert name.encode() in lib.isi_last_error() and b"null" in lib.isi_last_error()
    for name in ("N", "C", "K"):
        for bad in (0, -1):
            assert search(**{name: bad}) == -1 and (name.encode() + b" must be positive") in lib.isi_last_error()
    for bad in (0, -1, 65):
        assert search(Q=bad) == -1 and b"Q must lie in 1..64" in lib.isi_last_error()
    assert search(accumulate=2) == -1 and b"accumulate" in lib.isi_last_error()
    assert search(codes=FAKE + 1) == -1 and b"codes" in lib.isi_last_error()
    for name in ("weights", "table", "dist", "workspace"):
        assert search(**{name: FAKE + 2}) == -1 and name.encode() in lib.isi_last_error()
    assert search(K=16385) == -4 and b"K beyond 16384" in lib.isi_last_error()
    assert search(K=65536) == -4 and b"K beyond 65535" in lib.isi_last_error()
    assert search(C=256 * 65535 + 1) == -4 and b"C beyond" in lib.isi_last_error()
    need = lib.isi_code_search_workspace_bytes(1000, 1024, 512, 2)
    assert search(workspace_bytes=need - 1) == -3 and b"workspace_bytes" in lib.isi_last_error()
    assert search(workspace_bytes=0) == -3


class _Enc:                                      # stands in for sklearn's LabelEncoder
    def __init__(self, classes):
        self.classes = list(classes)

    def transform(self, values):
        return np.array([self.classes.index(v) for v in values])

    def inverse_transform(self, indexes):
        return np.array([self.classes[int(i)] for i in indexes], dtype=object)


def _vqvae(n_embed=32):
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    return VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
                 num_embeddings=n_embed, resolution_factors={"bottom": 4, "top": 2})


def test_code_index_validation_needs_no_device():
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.datasets.code_index import CodeIndex
    import inpainting
    vq = _vqvae()
    g = torch.Generator().manual_seed(0)
    top, bottom = torch.randint(0, 32, (20, 8, 4), generator=g), torch.randint(0, 32, (20, 16, 8), generator=g)
    encoders = {"pitch": _Enc(range(24, 85)), "instrument_family_str": _Enc([f"fam{i}" for i in range(11)])}
    attrs = {"pitch": torch.arange(20) + 12, "instrument_family_str": torch.arange(20) % 11}
    index = CodeIndex.from_arrays(top, bottom, attrs, vq, "cpu", encoders)
    assert len(index) == 20 and index.top.dtype == torch.uint16 and index.bottom.dtype == torch.uint16
    assert index.top_shape == (8, 4) and index.bottom_shape == (16, 8)
    t, b, a = index[7]
    assert t.dtype == torch.int64 and torch.equal(t, top[7]) and torch.equal(b, bottom[7])
    assert list(a) == ["pitch", "instrument_family_str"] and a["pitch"].shape == (1,) and int(a["pitch"]) == 19
    assert index.decoded_attributes(7) == {"pitch": 43, "instrument_family_str": "fam7", "pitch_class": 7, "octave": 3}
    with pytest.raises(IndexError):
        index[20]
    # out-of-range codes, bad shapes, disagreeing counts
    bad = top.clone()
    bad[3, 2, 1] = 32
    with pytest.raises(ValueError, match=r"\[0, 32\)"):
        CodeIndex.from_arrays(bad, bottom, attrs, vq, "cpu")
    bad[3, 2, 1] = -1
    with pytest.raises(ValueError):
        CodeIndex.from_arrays(bad, bottom, attrs, vq, "cpu")
    with pytest.raises(ValueError):
        CodeIndex.from_arrays(top, bottom[:19], attrs, vq, "cpu")
    with pytest.raises(ValueError):
        CodeIndex.from_arrays(top[0], bottom, attrs, vq, "cpu")
    with pytest.raises(ValueError):
        CodeIndex.from_arrays(top.float(), bottom, attrs, vq, "cpu")
    with pytest.raises(ValueError):
        CodeIndex.from_arrays(top, bottom, {"pitch": torch.arange(19)}, vq, "cpu")
    # one pass over a sequence of dataset items; ragged shapes and bad codes are refused
    items = [(top[i], bottom[i], {"pitch": attrs["pitch"][i:i + 1], "instrument_family_str": attrs["instrument_family_str"][i:i + 1]})
             for i in range(20)]
    again = CodeIndex.from_dataset(items, vq, "cpu", encoders)
    assert torch.equal(again.top, index.top) and torch.equal(again.bottom, index.bottom)
    assert all(torch.equal(again.attributes[k], index.attributes[k]) for k in attrs)
    ragged = list(items)
    ragged[5] = (top[5][:, :3], bottom[5][:, :6], items[5][2])
    with pytest.raises(ValueError, match="item 5"):
        CodeIndex.from_dataset(ragged, vq, "cpu")
    wrong = list(items)
    wrong[9] = (top[9], torch.full((16, 8), 40), items[9][2])
    with pytest.raises(ValueError, match="item 9"):
        CodeIndex.from_dataset(wrong, vq, "cpu")
    with pytest.raises(ValueError):
        CodeIndex.from_dataset([], vq, "cpu")
    # constraints: the decoded-attribute equality of sample_from_database, item by item
    for constraints in ({"pitch": 43}, {"pitch_class": 0}, {"octave": 3, "instrument_family_str": "fam2"}, {"pitch": 200},
                        {"instrument_family_str": "nope"}, {"unknown": 1}, {"pitch_class": 0, "octave": 4}):
        want = [all(k in index.decoded_attributes(i) and index.decoded_attributes(i)[k] == v for k, v in constraints.items())
                for i in range(20)]
        assert index.allowed(constraints).tolist() == [int(x) for x in want], constraints
    assert index.allowed() is None and index.allowed({}, []) is None
    assert index.allowed(None, [3, 19]).tolist() == [0 if i in (3, 19) else 1 for i in range(20)]
    # query validation comes before any device work; then: no CPU path
    with pytest.raises(ValueError):
        index.search()
    with pytest.raises(ValueError, match="top_code"):
        index.search(top[0][:, :3])
    with pytest.raises(ValueError, match="bottom_code"):
        index.search(top[0], bottom[0][:8])
    with pytest.raises(ValueError, match="mask_top"):
        index.search(top[0], mask_top=torch.zeros(8, 3, dtype=torch.bool))
    with pytest.raises(ValueError):
        index.search(top[0], k=0)
    with pytest.raises(ValueError):
        index.search(top[:3], bottom[:2])
    with pytest.raises(LookupError):                                   # nobody admitted: said before any upload or launch
        index.search(top[0], bottom[0], attribute_constraints={"pitch": 1000})
    with pytest.raises(_hip.HipLibraryError):
        index.search(top[0], bottom[0])
    with pytest.raises(_hip.HipLibraryError):
        inpainting.similar_sounds(index, top[:1], bottom[:1])
    with pytest.raises(ValueError):
        inpainting.sample_from_database(items, encoders, 4, {}, similar_to=(top[:1], bottom[:1]))
    with pytest.raises(ValueError):
        inpainting.similar_sounds(index, top[:1], bottom[:1], layer="middle")
    # without the new keywords sample_from_database is what it was
    (t4, b4), found = inpainting.sample_from_database(items, encoders, 4, {"pitch": 43}, torch.Generator().manual_seed(1))
    assert torch.equal(t4[0], top[7]) and torch.equal(b4[0], bottom[7]) and found["instrument_family_str"] == "fam7"
