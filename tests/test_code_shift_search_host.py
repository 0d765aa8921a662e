"""Host-side checks of the shift-invariant code search (csrc/code_shift_search.hip, `CodeIndex.search_shifted`,
`inpainting.paste_fragment`): the written specification (tests/code_shift_search_spec.py) against a brute-force quadruple
loop, its fp32 emulation against the aligned search's at W == T, mutants of the specification (so the GPU cases have
teeth), the C-ABI's refusals before any launch, what `search_shifted` validates without a device, and `paste_fragment` on
CPU tensors.  No GPU needed."""
import numpy as np
import pytest
import torch

import code_search_spec as S
import code_shift_search_spec as SS

FAKE = S.FAKE


def _case(N, F, T, W, K, Q, seed, integer=True):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, K, (N, F, T)).astype(np.uint16)
    query = rng.integers(0, K, (Q, F, W)).astype(np.uint16)
    if F * W > 1:
        query[rng.random((Q, F, W)) < 0.15] = K                      # the priors' mask token: counts nothing
    if integer:
        table = rng.integers(0, 256, (K, K)).astype(np.float32)       # asymmetric on purpose
        w = (rng.random((Q, F, W)) < 0.7).astype(np.float32)
    else:
        table = S.table64(rng.standard_normal((K, 8)).astype(np.float32)).astype(np.float32)
        w = (2.0 * rng.random((Q, F, W))).astype(np.float32)
    return codes, query, w, table


def test_spec_against_a_brute_force_quadruple_loop():
    N, F, T, W, K, Q, shift0, step, count = 4, 3, 11, 4, 6, 2, 1, 2, 4          # offsets 1, 3, 5, 7; 7 + 4 = 11 = T
    codes, query, w, table = _case(N, F, T, W, K, Q, 0)
    got, mag = SS.search64(codes, query, w, table, shift0, step, count)
    exact = SS.search_int(codes, query, w, table, shift0, step, count)
    assert got.shape == (Q, count, N) and (query == K).any()
    for j in range(Q):
        for s in range(count):
            for n in range(N):
                want = 0.0
                for f in range(F):
                    for t in range(W):
                        if query[j, f, t] < K:
                            want += float(w[j, f, t]) * float(table[query[j, f, t], codes[n, f, t + shift0 + s * step]])
                assert got[j, s, n] == want == exact[j, s, n] == mag[j, s, n]
    assert SS.offsets(shift0, step, count) == [1, 3, 5, 7]
    with pytest.raises(AssertionError):
        SS.search_int(codes, query, w, table, shift0, step, count + 1)          # offset 9: the window leaves the map
    # best offset: the first of equal minima; items that are not allowed
    dist = np.array([[[3., 1., 5.], [2., 1., 5.], [2., 4., 0.]]])               # [1, S = 3, N = 3]
    value, shift = SS.best(dist, np.array([1, 1, 0]))
    assert value.tolist() == [[2., 1., np.inf]] and shift.tolist() == [[1, 0, -1]] and shift.dtype == np.int32
    assert SS.best(dist)[1].tolist() == [[1, 0, 2]]


def test_emulation_at_full_width_is_the_aligned_search_bit_for_bit():
    N, F, T, K, Q = 20, 5, 60, 64, 2                                  # F * T = 300: a second run of 44 cells
    codes, query, w, table = _case(N, F, T, T, K, Q, 1, integer=False)
    got = SS.emulate(codes, query, w, table, 0, 1, 1)
    want = S.emulate_f32(codes.reshape(N, F * T), query.reshape(Q, F * T), w.reshape(Q, F * T), table)
    assert got.shape == (Q, 1, N) and np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32))
    # narrower windows: inside the bound with C = F * W, and exact on integer tables
    W = 52
    ref, mag = SS.search64(codes, query[:, :, :W], w[:, :, :W], table, 2, 3, 3)
    err = np.abs(SS.emulate(codes, query[:, :, :W], w[:, :, :W], table, 2, 3, 3).astype(np.float64) - ref)
    assert (err <= SS.bound(mag, F, W)).all() and err.max() > 0
    codes, query, w, table = _case(N, F, T, W, K, Q, 2)
    assert np.array_equal(SS.emulate(codes, query, w, table, 0, 4, 3).astype(np.int64),
                          SS.search_int(codes, query, w, table, 0, 4, 3))


def test_mutants_of_the_specification_violate_it():
    """What the GPU cases would catch: each mutant differs from the specification on the exact cases' kind of input."""
    N, F, T, W, K, Q, shift0, step, count = 30, 3, 40, 9, 64, 2, 2, 2, 5
    codes, query, w, table = _case(N, F, T, W, K, Q, 3)
    want = SS.search_int(codes, query, w, table, shift0, step, count)
    offs = SS.offsets(shift0, step, count)

    def terms(q_cols, c_cols):
        """sum over f and the paired columns (query column, stored column) of w T[q][x], as int64 [Q, N]."""
        out = np.zeros((Q, N), np.int64)
        for j in range(Q):
            for tq, tc in zip(q_cols, c_cols):
                q = query[j, :, tq].astype(np.int64)
                live = (q < K) & (w[j, :, tq] > 0)
                out[j] += (table[np.where(live, q, 0)[None, :], codes[:, :, tc]].astype(np.int64) * live[None, :]).sum(1)
        return out
    right = np.stack([terms(range(W), range(o, o + W)) for o in offs], 1)
    assert np.array_equal(right, want)                                # the helper itself is the specification
    # the offset applied to the query instead of the stored map: query column (t + o) % W against stored column t
    on_query = np.stack([terms([(t + o) % W for t in range(W)], range(W)) for o in offs], 1)
    assert (on_query != want).any()
    # t - o instead of t + o (stored columns taken modulo T, so that the mutant reads inside the map)
    minus = np.stack([terms(range(W), [(t - o) % T for t in range(W)]) for o in offs], 1)
    assert (minus != want).any()
    # ties to the largest s
    dist = want.astype(np.float64).copy()
    dist[:, 3, :] = dist[:, 1, :] = dist.min(1) - 1                   # planted ties at s = 1 and s = 3
    value, shift = SS.best(dist)
    assert (shift == 1).all()
    largest = (dist.shape[1] - 1 - np.argmin(dist[:, ::-1, :], axis=1)).astype(np.int32)
    assert (largest == 3).all() and (largest != shift).all()
    # a run boundary at 255 instead of 256 moves float bits (and an integer case cannot see it)
    N, F, T, W, K = 64, 4, 130, 128, 64                               # F * W = 512: two runs
    codes, query, w, table = _case(N, F, T, W, K, 1, 4, integer=False)
    good = SS.emulate(codes, query, w, table, 1, 1, 2)
    old = S.RUN
    try:
        S.RUN = 255
        bad = SS.emulate(codes, query, w, table, 1, 1, 2)
    finally:
        S.RUN = old
    assert (good.view(np.uint32) != bad.view(np.uint32)).any()
    assert np.array_equal(SS.emulate(codes, query, w, table, 1, 1, 2).view(np.uint32), good.view(np.uint32))


def test_cabi_refusals_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    ws = lib.isi_code_shift_search_workspace_bytes
    assert ws(1000, 16, 64, 16, 49, 512, 1) == 16                     # one run: dist is written directly
    assert ws(1000, 32, 128, 32, 49, 512, 2) == 4 * 2 * 49 * 1000 * 4
    assert ws(64, 1, 300, 257, 44, 64, 1) == 2 * 1 * 44 * 64 * 4
    assert ws(305979, 32, 128, 32, 49, 512, 8) == 4 * 8 * 49 * 305979 * 4
    assert ws(0, 16, 64, 16, 49, 512, 1) == 0 and ws(10, 16, 64, 16, 49, 512, 65) == 0 and ws(10, 16, 64, 65, 1, 512, 1) == 0
    ok = dict(codes=FAKE, query=FAKE, weights=FAKE, table=FAKE, dist=FAKE, N=1000, F=32, T=128, W=32, shift0=0, step=2, S=49,
              K=512, Q=2, accumulate=0, workspace=FAKE, workspace_bytes=1 << 30)

    def search(**kw):
        a = dict(ok, **kw)
        return lib.isi_code_shift_search_f32(a["codes"], a["query"], a["weights"], a["table"], a["dist"], a["N"], a["F"],
                                             a["T"], a["W"], a["shift0"], a["step"], a["S"], a["K"], a["Q"], a["accumulate"],
                                             a["workspace"], a["workspace_bytes"], None)
    for name in ("codes", "query", "table", "dist", "workspace"):
        assert search(**{name: None}) == -1
        assert name.encode() in lib.isi_last_error() and b"null" in lib.isi_last_error()
    for name in ("N", "F", "T", "W", "S", "K", "step"):
        for bad in (0, -1):
            assert search(**{name: bad}) == -1 and (name.encode() + b" must be positive") in lib.isi_last_error(), name
    assert search(shift0=-1) == -1 and b"shift0" in lib.isi_last_error()
    assert search(W=129) == -1 and b"W must not exceed T" in lib.isi_last_error()
    assert search(S=50) == -1 and b"shift0 + (S - 1) * step + W" in lib.isi_last_error()          # 98 + 32 > 128
    assert search(shift0=1) == -1 and b"shift0 + (S - 1) * step + W" in lib.isi_last_error()
    assert search(step=3) == -1 and b"shift0 + (S - 1) * step + W" in lib.isi_last_error()
    for bad in (0, -1, 65):
        assert search(Q=bad) == -1 and b"Q must lie in 1..64" in lib.isi_last_error()
    for bad in (2, -1):
        assert search(accumulate=bad) == -1 and b"accumulate" in lib.isi_last_error()
    for name in ("codes", "query"):
        assert search(**{name: FAKE + 1}) == -1 and name.encode() in lib.isi_last_error()
    for name in ("weights", "table", "dist", "workspace"):
        assert search(**{name: FAKE + 2}) == -1 and name.encode() in lib.isi_last_error()
    assert search(weights=None, workspace_bytes=0) == -3             # null weights are fine: 1 on every cell
    assert search(K=16385) == -4 and b"K beyond 16384" in lib.isi_last_error()
    assert search(K=65536) == -4 and b"K beyond 65535" in lib.isi_last_error()
    wide = dict(F=4, T=256 * 65535, W=256 * 65535 // 4 + 1, S=1, step=1)
    assert search(**wide) == -4 and b"F * W beyond" in lib.isi_last_error()
    assert search(F=1 << 20, T=1 << 11, W=8, S=1, step=1) == -4 and b"F * T beyond" in lib.isi_last_error()
    assert search(N=1 << 33, Q=64, S=1, step=1) == -4 and b"Q * S * N beyond" in lib.isi_last_error()
    assert search(N=(1 << 39) - 1, F=16, T=64, W=16, Q=1, S=1, step=1) == -4 and b"workgroups" in lib.isi_last_error()      # 2^31 blocks of 256 items
    need = ws(1000, 32, 128, 32, 49, 512, 2)
    assert search(workspace_bytes=need - 1) == -3 and b"workspace_bytes" in lib.isi_last_error()
    assert search(workspace_bytes=0) == -3
    assert search(F=16, T=64, W=16, step=1, workspace_bytes=15) == -3                             # one run: 16 bytes
    # the best-offset pass
    okb = dict(dist=FAKE, allowed=FAKE, best=FAKE, best_shift=FAKE, N=1000, S=49, Q=2)

    def best(**kw):
        a = dict(okb, **kw)
        return lib.isi_code_shift_best_f32(a["dist"], a["allowed"], a["best"], a["best_shift"], a["N"], a["S"], a["Q"], None)
    for name in ("dist", "best", "best_shift"):
        assert best(**{name: None}) == -1 and name.encode() in lib.isi_last_error() and b"null" in lib.isi_last_error()
        assert best(**{name: FAKE + 2}) == -1 and name.encode() in lib.isi_last_error()
    for name in ("N", "S"):
        for bad in (0, -1):
            assert best(**{name: bad}) == -1 and (name.encode() + b" must be positive") in lib.isi_last_error()
    for bad in (0, 65):
        assert best(Q=bad) == -1 and b"Q must lie in 1..64" in lib.isi_last_error()
    assert best(N=1 << 33, Q=64) == -4 and b"Q * S * N beyond" in lib.isi_last_error()


class _Enc:                                      # stands in for sklearn's LabelEncoder
    def __init__(self, classes):
        self.classes = list(classes)

    def transform(self, values):
        return np.array([self.classes.index(v) for v in values])

    def inverse_transform(self, indexes):
        return np.array([self.classes[int(i)] for i in indexes], dtype=object)


def test_search_shifted_validation_needs_no_device():
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.datasets.code_index import CodeIndex
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    import inpainting
    vq = VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
               num_embeddings=32, resolution_factors={"bottom": 4, "top": 2})
    g = torch.Generator().manual_seed(0)
    top, bottom = torch.randint(0, 32, (20, 8, 6), generator=g), torch.randint(0, 32, (20, 16, 12), generator=g)
    index = CodeIndex.from_arrays(top, bottom, {"pitch": torch.arange(20) + 12}, vq, "cpu", {"pitch": _Enc(range(24, 85))})
    q_top, q_bottom = top[0][:, 1:4], bottom[0][:, 2:8]
    with pytest.raises(ValueError):
        index.search_shifted()
    with pytest.raises(ValueError, match="top_code"):
        index.search_shifted(top[0][:7, :3])                          # rows disagree with the stored maps
    with pytest.raises(ValueError, match="top_code"):
        index.search_shifted(torch.cat([top[0], top[0]], -1))         # wider than the stored maps
    with pytest.raises(ValueError, match="top_code"):
        index.search_shifted(q_top.float())
    with pytest.raises(ValueError, match="bottom_code"):
        index.search_shifted(q_top, bottom[0][:, 2:7])                # 5 bottom columns under 3 top columns
    with pytest.raises(ValueError, match="mask_top"):
        index.search_shifted(q_top, mask_top=torch.zeros(8, 6, dtype=torch.bool))      # the stored shape, not the window's
    with pytest.raises(ValueError):
        index.search_shifted(q_top, k=0)
    with pytest.raises(ValueError):
        index.search_shifted(torch.stack([q_top] * 3), torch.stack([q_bottom] * 2))
    with pytest.raises(ValueError, match="shift_range"):
        index.search_shifted(q_top, shift_range=(4, 9))               # a window of 3 fits at 0..3 only
    with pytest.raises(ValueError, match="shift_range"):
        index.search_shifted(q_top, shift_range=(2, 2))
    with pytest.raises(ValueError):
        index.search_shifted(q_top, layer_weights=(1.0, -1.0))
    with pytest.raises(LookupError):
        index.search_shifted(q_top, attribute_constraints={"pitch": 1000})
    # then: no CPU path
    with pytest.raises(_hip.HipLibraryError):
        index.search_shifted(q_top, q_bottom)
    with pytest.raises(_hip.HipLibraryError):
        index.distances_shifted(bottom_code=q_bottom)
    with pytest.raises(_hip.HipLibraryError):
        inpainting.similar_fragments(index, top[:1], bottom[:1], 1, 3)
    with pytest.raises(ValueError):
        inpainting.similar_fragments(index, top[:1], bottom[:1], 4, 3)                 # the window leaves the sound
    with pytest.raises(ValueError):
        inpainting.similar_fragments(index, top[:1], bottom[:1], 1, 3, layer="middle")
    with pytest.raises(ValueError, match="mask"):
        inpainting.similar_fragments(index, top[:1], bottom[:1], 1, 3, mask=torch.zeros(1, 8, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="nothing is masked"):
        inpainting.patch_from_database(index, top[:1], bottom[:1], torch.zeros(1, 8, 6, dtype=torch.bool))


def test_paste_fragment_on_cpu_tensors():
    import inpainting
    F_t, T, F_b, T_b = 2, 6, 4, 12                                    # both ratios 2
    top = torch.arange(F_t * T).reshape(1, F_t, T)
    bottom = torch.arange(F_b * T_b).reshape(1, F_b, T_b)
    item_top = 100 + torch.arange(F_t * 5).reshape(1, F_t, 5)          # an item of 5 top / 10 bottom columns
    item_bottom = 1000 + torch.arange(F_b * 10).reshape(1, F_b, 10)
    # window = top columns 2..4; the hole: row 0 of columns 2 and 3, row 1 of column 4; item column = col - 2 + 3
    mask = torch.tensor([[[True, True, False], [False, False, True]]])
    new_top, new_bottom = inpainting.paste_fragment(top, bottom, item_top, item_bottom, mask, "top", 2, 3)
    want_top = top.clone()
    want_top[0, 0, 2], want_top[0, 0, 3] = item_top[0, 0, 3], item_top[0, 0, 4]
    # (top column 4 would take item column 5: outside the item, unchanged)
    assert torch.equal(new_top, want_top) and new_top is not top and torch.equal(top, torch.arange(F_t * T).reshape(1, F_t, T))
    want_bottom = bottom.clone()
    for row in (0, 1):                                                # top row 0 -> bottom rows 0, 1; top columns 2, 3 -> bottom 4..7
        for col in range(4, 8):
            want_bottom[0, row, col] = item_bottom[0, row, col - 4 + 6]
    # (top row 1, column 4 -> bottom rows 2, 3, columns 8, 9 -> item columns 10, 11: outside the item, unchanged)
    assert torch.equal(new_bottom, want_bottom)
    # shift 0: the third cell has a source now
    new_top, new_bottom = inpainting.paste_fragment(top, bottom, item_top, item_bottom, mask, "top", 2, 0)
    assert new_top[0].tolist() == [[0, 1, 100, 101, 4, 5], [6, 7, 8, 9, 107, 11]]
    assert new_bottom[0, 2:, 8:10].tolist() == [[1024, 1025], [1034, 1035]] and new_bottom[0, 0, 4:8].tolist() == [1000, 1001, 1002, 1003]
    assert torch.equal(new_bottom[0, :, :4], bottom[0, :, :4]) and torch.equal(new_bottom[0, :2, 8:], bottom[0, :2, 8:])
    # a bottom-layer mask leaves the top map alone; a window that starts left of the item (negative source) changes nothing there
    mask_b = torch.zeros(1, F_b, 4, dtype=torch.bool)
    mask_b[0, 3, :] = True
    new_top, new_bottom = inpainting.paste_fragment(top, bottom, item_top, item_bottom, mask_b, "bottom", 1, 0)
    assert torch.equal(new_top, top) and new_bottom[0, 3, 2:6].tolist() == [1030, 1031, 1032, 1033]
    assert int((new_bottom != bottom).sum()) == 4
    new_top, new_bottom = inpainting.paste_fragment(top, bottom, item_top, item_bottom, mask_b, "bottom", 1, -1)
    assert new_bottom[0, 3, 2:6].tolist() == [38, 39, 1030, 1031]     # item columns -2, -1 do not exist
    with pytest.raises(ValueError):
        inpainting.paste_fragment(top, bottom, item_top, item_bottom, mask, "bottom", 2, 0)      # a top-shaped mask
    with pytest.raises(ValueError):
        inpainting.paste_fragment(top, bottom, item_top, item_bottom, mask, "side", 2, 0)
