"""The top-M / palette-restricted codebook search without a GPU: the float64 specification (tests/vq_topm_spec.py) against
a brute-force torch.topk / sort and against its own edge rules, the fp32 model of the kernel inside the comparison the GPU
file uses, that comparison against planted faults, `pack_palettes`' bit layout, `VQVAE.soft_weights`, and every refusal of
isi_vq_nearest_topm_f32 (the library loads without a GPU and refuses before any launch)."""
import pytest
import torch

import vq_topm_spec as S

INF, NAN = float("inf"), float("nan")


# --------------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("N,D,K,M", [(40, 8, 40, 1), (64, 16, 77, 5), (50, 64, 512, 8)])
def test_spec_equals_brute_force_topk(N, D, K, M):
    g = torch.Generator().manual_seed(N + K)
    z, E = torch.randn(N, D, generator=g), torch.randn(K, D, generator=g)
    allowed = torch.rand(3, K, generator=g) < 0.4
    rows = torch.randint(0, 3, (N,), generator=g)
    for al, ar in ((None, None), (allowed, None), (allowed, rows)):
        ids, dist = S.topm_spec(z, E, M, al, ar)
        d = (z.double()[:, None, :] - E.double()[None]).pow(2).sum(-1)                 # the definition, term by term
        if al is not None:
            d = d.masked_fill(~al[rows if ar is not None else torch.zeros(N, dtype=torch.long)], INF)
        vals, idx = d.topk(M, dim=1, largest=False)
        assert torch.equal(ids, idx.T)                                                 # random data: no ties
        assert torch.allclose(dist, vals.T, rtol=0, atol=1e-12 * float(d[d < INF].max()))
        srt = d.sort(1)
        assert torch.equal(ids, srt.indices[:, :M].T)


def test_spec_edge_rules():
    E = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [NAN, 0.0], [0.0, 3.0], [INF, 1.0]])
    z = torch.tensor([[1.0, 0.0], [0.0, 2.9], [NAN, 0.0], [0.0, -INF], [0.4, 0.0]])
    ids, dist = S.topm_spec(z, E, 5)
    assert ids[:, 0].tolist() == [1, 2, 0, 4, -1]          # duplicates 1 = 2: the lower first; codes 3 and 5 never returned
    assert dist[:, 0].tolist() == [0.0, 0.0, 1.0, 10.0, INF]
    assert ids[:, 1].tolist() == [4, 0, 1, 2, -1]
    for lost in (2, 3):                                    # a NaN / an Inf component
        assert ids[:, lost].tolist() == [-1] * 5 and bool(torch.isnan(dist[:, lost]).all())
    assert ids[:3, 4].tolist() == [0, 1, 2]                # 0.16 < 0.36 = 0.36
    allowed = torch.tensor([[True] * 6, [False, False, True, True, False, True], [False] * 6])
    ids, dist = S.topm_spec(z, E, 3, allowed, torch.tensor([1, 0, 1, 2, 3]))
    assert ids[:, 0].tolist() == [2, -1, -1] and dist[:, 0].tolist() == [0.0, INF, INF]      # one finite code in the palette
    assert ids[:, 1].tolist() == [4, 0, 1]
    assert ids[:, 3].tolist() == [-1] * 3 and bool(torch.isnan(dist[:, 3]).all())            # lost beats the empty palette
    assert ids[:, 4].tolist() == [-1] * 3 and dist[:, 4].tolist() == [INF] * 3               # row 3 of 3: empty palette
    free = S.near_tie_free(z, E)
    assert free.tolist() == [True, True, True, True, True]           # codes 1 = 2 are one vector: the index rule, not a near-tie
    assert S.near_tie_free(torch.tensor([[0.5, 0.0], [0.5 + 1e-6, 0.0]]), E).tolist() == [False, False]   # between codes 0 and 1
    assert S.near_tie_free(torch.tensor([[0.5, 0.0]]), E, torch.tensor([[True, False, False, False, True, False]])).tolist() == [True]


# ------------------------------------------------------------------------- the model of the kernel, and the comparison
HOST_CASES = [(257, 64, 512), (257, 64, 77), (33, 8, 40), (1, 64, 512)]


@pytest.mark.parametrize("palettes", [False, True])
@pytest.mark.parametrize("N,D,K", HOST_CASES)
def test_fp32_model_passes_the_comparison(N, D, K, palettes):
    case = S.make_case(N, D, K, palettes=palettes)
    share, kept = S.rejected_share(case)
    assert share <= S.MAX_REJECTED, f"{share:.3%} of the vectors are near-ties"
    for M in (1, 2, 5, 8):
        ids_buf, dist_buf = S.model_f32(case, M)
        ratio, swaps = S.compare(ids_buf, dist_buf, case, M, f"model N={N} D={D} K={K} M={M}", kept)
        assert ratio <= 1.0
        S.check_duplicates(ids_buf, dist_buf, case, M)


def test_rejected_share_at_the_measured_sizes():
    """K = 512, D = 64: the share of vectors with a near-tie among their nine nearest allowed codes stays under the cap, with
    the full codebook and with a palette of about 50 codes"""
    case = S.make_case(20011, 64, 512, palettes=False)
    share, _ = S.rejected_share(case)
    assert share <= S.MAX_REJECTED
    g = torch.Generator().manual_seed(3)
    small = (torch.rand(1, 512, generator=g) < 54 / 512)
    free = S.near_tie_free(case.z[~case.planted], case.E, small, None)
    assert float((~free).float().mean()) <= S.MAX_REJECTED


@pytest.mark.parametrize("fault", S.FAULTS)
def test_comparison_rejects_planted_faults(fault):
    caught = 0
    for N, D, K in ((257, 64, 77), (33, 8, 40)):
        case = S.make_case(N, D, K, palettes=True)
        kept = S.rejected_share(case)[1]
        for M in (2, 5):
            S.compare(*S.model_f32(case, M), case, M, "clean", kept)
            ids_buf, dist_buf = S.model_f32(case, M, fault)
            try:
                S.compare(ids_buf, dist_buf, case, M, fault, kept)
                S.check_duplicates(ids_buf, dist_buf, case, M, fault)
            except AssertionError:
                caught += 1
    assert caught == 4, f"{fault} slipped through {4 - caught} of 4 comparisons"


# ------------------------------------------------------------------------------------------------------------ palettes
@pytest.mark.parametrize("K", [77, 512, 32, 1])
def test_pack_palettes_bit_layout_and_round_trip(K):
    from interactive_spectrogram_inpainting.vqvae import _ops
    g = torch.Generator().manual_seed(K)
    table = torch.rand(5, K, generator=g) < 0.3
    table[3] = False
    table[4] = True
    words = _ops.pack_palettes(table, K)
    W = (K + 31) // 32
    assert words.dtype == torch.int32 and tuple(words.shape) == (5, W)
    for p in range(5):
        for k in range(K):
            assert bool((int(words[p, k >> 5]) >> (k & 31)) & 1) == bool(table[p, k])
        for k in range(K, W * 32):                                   # nothing beyond K
            assert not (int(words[p, k >> 5]) >> (k & 31)) & 1
    assert torch.equal(_ops.unpack_palettes(words, K), table)
    # the other forms: one bool row (sample.codes_in_use), a list of index tensors / bool rows
    assert torch.equal(_ops.pack_palettes(table[0], K), words[:1])
    as_list = [table[0].nonzero().flatten(), table[1], table[2].nonzero().flatten().tolist(), torch.zeros(0, dtype=torch.int64), table[4]]
    assert torch.equal(_ops.pack_palettes(as_list, K), words)
    import sample
    used = sample.codes_in_use(torch.tensor([[0, K - 1, K, -1]]), K)
    assert _ops.unpack_palettes(_ops.pack_palettes(used, K), K)[0].nonzero().flatten().tolist() == sorted({0, K - 1})
    for bad in (torch.zeros(K + 1, dtype=torch.bool), torch.zeros(2, K), [torch.tensor([K])], [torch.tensor([-1])], [], [torch.tensor([0.5])]):
        with pytest.raises(ValueError):
            _ops.pack_palettes(bad, K)


# -------------------------------------------------------------------------------------------------------- soft weights
def test_soft_weights_rules():
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    g = torch.Generator().manual_seed(0)
    d = torch.rand(8, 3, 50, generator=g).cumsum(0) * 20                 # non-decreasing along M
    d[5:, 0, :10] = INF                                                  # short palettes: ranks 5.. missing
    d[:, 1, 3] = INF                                                     # an empty palette
    d[:, 2, 4] = NAN                                                     # a non-finite vector
    for T in (0.05, 1.0, 30.0, 1e6):
        w = VQVAE.soft_weights(d, T)
        assert w.dtype == torch.float32 and w.shape == d.shape and bool(torch.isfinite(w).all()) and bool((w >= 0).all())
        assert bool((w[5:, 0, :10] == 0).all()) and bool((w[:, 1, 3] == 0).all()) and bool((w[:, 2, 4] == 0).all())
        live = torch.ones(3, 50, dtype=torch.bool)
        live[1, 3] = live[2, 4] = False
        assert bool(((w.sum(0) - 1).abs()[live] <= 8 * 2.0 ** -23).all())          # a few ulp of 1
        assert bool((w[:-1] >= w[1:]).all())                                        # nearer codes weigh more
        want = torch.softmax(-(d.double() - d[:1].double()) / T, 0)                  # (inf ranks: exp(-inf) = 0)
        assert torch.allclose(w[:, live].double(), want[:, live], rtol=1e-5, atol=1e-7)
    w0 = VQVAE.soft_weights(d, 0)
    assert bool((w0[0][live] == 1).all()) and bool((w0[1:] == 0).all()) and bool((w0[0][~live] == 0).all())
    for bad in (-1.0, -0.0001, NAN):
        with pytest.raises(ValueError):
            VQVAE.soft_weights(d, bad)


def test_model_entry_points_refuse_what_they_cannot_do():
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    from interactive_spectrogram_inpainting.vqvae.bottleneck import UnquantizedBottleneck
    import inpainting
    small = dict(in_channel=2, num_hidden_channels=32, num_residual_channels=8, embed_dim=16, num_embeddings=64)
    x = torch.randn(1, 2, 16, 16)
    with pytest.raises(RuntimeError, match="eval"):
        VQVAE(**small).train().encode_topm(x)
    with pytest.raises(NotImplementedError):
        VQVAE(**small, disable_quantization=True).eval().encode_topm(x)
    with pytest.raises(NotImplementedError):
        UnquantizedBottleneck(16, 64).nearest_codes(torch.randn(1, 2, 2, 16))
    m = VQVAE(**small).eval()
    with pytest.raises(ValueError, match="allows no code"):
        inpainting.render_with_palette(m, x, torch.zeros(64, dtype=torch.bool))
    with pytest.raises(ValueError, match="layer"):
        inpainting.code_alternatives(m, x, 2, "middle")


# ------------------------------------------------------------------------------------------ refusals before any launch
def test_topm_refuses_bad_arguments_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    ok, odd = 0x10000, 0x10004        # non-null, never dereferenced on the host: 16-byte aligned / 4 bytes off
    INVALID, UNSUPPORTED = -1, -4
    good = dict(z=ok, codes=ok, e2=ok, allowed=ok, P=4, allowed_row=ok, ids=ok, ids_stride=10, dist=ok, dist_stride=10, N=10,
                D=64, K=512, M=4)

    def call(**change):
        a = dict(good, **change)
        return L.isi_vq_nearest_topm_f32(a["z"], a["codes"], a["e2"], a["allowed"], a["P"], a["allowed_row"], a["ids"],
                                         a["ids_stride"], a["dist"], a["dist_stride"], a["N"], a["D"], a["K"], a["M"], None)

    def refused(rc, message, code=INVALID):
        assert rc == code
        assert message in L.isi_last_error(), L.isi_last_error()

    for name in ("z", "codes", "e2", "ids", "dist"):
        refused(call(**{name: None}), b"vq_topm: null pointer")
    for N in (0, -3):
        refused(call(N=N), b"vq_topm: N must be positive")
    for M in (0, 9, -1):
        refused(call(M=M), b"vq_topm: M must be 1..8")
    for D in (0, 4, 24, 128, -8):
        refused(call(D=D), b"vq_topm: D must be 8, 16, 32 or 64")
    for K in (0, -1):
        refused(call(K=K), b"vq_topm: K must be positive")
    strides = b"vq_topm: ids_stride and dist_stride must be at least N"
    refused(call(ids_stride=9), strides)
    refused(call(dist_stride=9), strides)
    refused(call(dist_stride=-10), strides)
    refused(call(allowed=None, P=0), b"vq_topm: allowed_row given without allowed")
    refused(call(allowed=None, allowed_row=None, P=4), b"vq_topm: P must be 0 without allowed")
    for P in (0, -1):
        refused(call(P=P), b"vq_topm: P must be positive with allowed")
    refused(call(z=odd), b"vq_topm: z and codes must be 16-byte aligned")
    refused(call(codes=odd), b"vq_topm: z and codes must be 16-byte aligned")
    # beyond what stays on chip
    refused(call(P=65), b"vq_topm: at most 64 palette rows", UNSUPPORTED)
    lds = b"vq_topm: codebook and palettes do not fit in LDS"
    refused(call(K=1000), lds, UNSUPPORTED)                              # as isi_vq_nearest_f32 at D = 64
    refused(call(K=1000, allowed=None, allowed_row=None, P=0), lds, UNSUPPORTED)
    refused(call(K=544, P=64), lds, UNSUPPORTED)           # 544 codes alone fit (152 352 bytes), not with 64 palette rows beside
    refused(call(N=1 << 40, ids_stride=1 << 40, dist_stride=1 << 40), b"vq_topm: N must stay below 2^40", UNSUPPORTED)
    refused(call(ids_stride=1 << 56), b"vq_topm: N must stay below 2^40", UNSUPPORTED)
