"""isi_vq_nearest_topm_f32 (csrc/vq_topm.hip) against its float64 specification (tests/vq_topm_spec.py, which also holds
the test data and the comparison), and the public path above it: VQVAE.encode_topm, inpainting.render_with_palette /
encode_soft / code_alternatives.

Kernel cases, the smallest at which this kernel can go wrong: N in {1, 33, 257, 20011} (one lane; one past a wave's 32
vectors; one past a workgroup pass of 256; 79 workgroups, the last one ragged -- and once N = 65 836 at the smallest shape,
where the 256 persistent workgroups take a second, ragged pass), (D, K) in {(64, 512),
(64, 77), (8, 40)} (the real codebook; padding codes in the last tile; the smallest D), M in {1, 2, 5, 8}, with and without
the four-row palette table of the spec's data (everything / a random row / exactly 3 codes / empty, rows -1 and P among
the vectors' rows, bits beyond K set).  The data holds two pairs of duplicated codes with vectors placed on them, a NaN and
an Inf vector, a NaN and an Inf code.  The outputs are flat poisoned buffers read through strides longer than N.
Asserted per case: vq_topm_spec.compare (exact ids on the near-tie-free vectors, certified near-ties elsewhere, the
distance bound (D + 3) 2^-24 S, -1 / +inf / NaN rules, palette membership, poison intact), the share of rejected vectors
<= 2 %, the duplicates' order.

A recording aid, not a check: with ISI_VQ_TOPM_RECORD=<file> in the environment the worst distance error / bound ratio and
the number of certified swaps of every kernel case are written there when the module ends."""
import functools
import os

import pytest
import torch

import vq_topm_spec as S

pytestmark = pytest.mark.gpu

RECORD = []
SHAPES = [(64, 512), (64, 77), (8, 40), (32, 77), (16, 200)]
SIZES = [1, 33, 257, 20011]
RANKS = [1, 2, 5, 8]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_VQ_TOPM_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# isi_vq_nearest_topm_f32 against the float64 spec, per case of tests/test_vq_topm_gpu.py: worst distance error /\n"
                "# bound ((D + 3) 2^-24 S, tests/vq_topm_spec.py), certified near-tie swaps, rejected share of the vectors\n")
        for ratio, swaps, share, what in sorted(RECORD, key=lambda r: -r[0]):
            f.write(f"{ratio:8.4f}  swaps {swaps:3d}  rejected {share:6.2%}  {what}\n")


@functools.lru_cache(maxsize=None)
def _case(N, D, K, palettes):
    return S.make_case(N, D, K, palettes=palettes)


def _packed(case):
    """(codes [K, D], e2 [K]) of the case's codebook on the device, by isi_pack_codebook_f32"""
    from interactive_spectrogram_inpainting.vqvae import _ops
    if not hasattr(case, "_dev_codes"):
        case._dev_codes = _ops.pack_codebook(case.E.T.contiguous().to(_dev()))
    return case._dev_codes


def _launch(case, M, z=None, rows=None, use_palette=None):
    """the kernel on the case's data (or on other vectors `z` / rows): flat poisoned host buffers (ids, dist)"""
    from interactive_spectrogram_inpainting import _hip
    L, dev = _hip.lib(), _dev()
    codes, e2 = _packed(case)
    z = case.z if z is None else z
    N = z.shape[0]
    use_palette = (case.allowed is not None) if use_palette is None else use_palette
    zd = z.to(dev)
    words = rows_d = None
    if use_palette:
        w = S.palette_words(case)
        words = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).to(dev)
        r = case.allowed_row if rows is None else rows
        rows_d = r.to(torch.int32).to(dev)
    ids_stride, dist_stride = (case.ids_stride, case.dist_stride) if N == case.N else (N + 3, N + 5)
    ids = torch.full((M * ids_stride + 11,), S.ID_POISON, dtype=torch.int64, device=dev)
    dist = torch.full((M * dist_stride + 11,), S.DIST_POISON, dtype=torch.int32, device=dev)
    rc = L.isi_vq_nearest_topm_f32(zd.data_ptr(), codes.data_ptr(), e2.data_ptr(), words.data_ptr() if use_palette else None,
                                   case.P if use_palette else 0, rows_d.data_ptr() if use_palette else None, ids.data_ptr(),
                                   ids_stride, dist.data_ptr(), dist_stride, N, case.D, case.K, M, _hip.stream_ptr(dev))
    assert rc == 0, L.isi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(zd.cpu().view(torch.int32), z.view(torch.int32)), "the kernel changed its input"
    return ids.cpu(), dist.cpu().view(torch.float32)


@pytest.mark.parametrize("palettes", [False, True], ids=["all_codes", "palettes"])
@pytest.mark.parametrize("D,K", SHAPES)
@pytest.mark.parametrize("N", SIZES)
def test_kernel_against_the_spec(N, D, K, palettes):
    case = _case(N, D, K, palettes)
    share, kept = S.rejected_share(case)
    print(f"N={N} D={D} K={K} palettes={palettes}: rejected share {share:.3%}, kept {int(kept.sum())}")
    assert share <= S.MAX_REJECTED, f"{share:.3%} of the vectors are near-ties"
    for M in RANKS:
        what = f"N={N} D={D} K={K} M={M} {'palettes' if palettes else 'all codes'}"
        ids_buf, dist_buf = _launch(case, M)
        ratio, swaps = S.compare(ids_buf, dist_buf, case, M, what, kept)
        print(f"  {what}: worst distance error / bound {ratio:.4f}, certified swaps {swaps}")
        S.check_duplicates(ids_buf, dist_buf, case, M, what)
        RECORD.append((ratio, swaps, share, what))
        if palettes and M >= 5 and N >= 33:                   # the three-code row leaves ranks 3.. empty
            ids = S.unpack(ids_buf, case.ids_stride, N, M, S.ID_POISON, what)
            three = case.allowed_row == 2
            assert bool(three.any()) and bool((ids[:3, three] >= 0).all()) and bool((ids[3:, three] == -1).all())
            assert bool((ids[:, (case.allowed_row == 3) | (case.allowed_row == -1) | (case.allowed_row == 4)] == -1).all())


def test_second_pass_of_the_persistent_workgroups():
    """N beyond 256 workgroups x 256 vectors: workgroups 0 and 1 loop a second time, the second one ragged"""
    N, D, K = 65536 + 300, 8, 40
    case = _case(N, D, K, True)
    share, kept = S.rejected_share(case)
    assert share <= S.MAX_REJECTED
    for M in (1, 8):
        ids_buf, dist_buf = _launch(case, M)
        S.compare(ids_buf, dist_buf, case, M, f"N={N} M={M} two passes", kept)
        S.check_duplicates(ids_buf, dist_buf, case, M)


@pytest.mark.parametrize("D,K", SHAPES)
@pytest.mark.parametrize("N", SIZES)
def test_rank_0_is_the_exact_search_index_for_index(N, D, K):
    """no palette: rank 0 equals isi_vq_nearest_f32's indices on UNFILTERED data -- near-ties, duplicates, the NaN and Inf
    vectors (-1) and the non-finite codes included -- and the distance is the one that search minimises"""
    from interactive_spectrogram_inpainting.vqvae import _ops
    case = _case(N, D, K, False)
    codes, e2 = _packed(case)
    _, _, idx, _ = _ops.vq_nearest(case.z.to(_dev()), codes, e2)
    for M in (1, 8):
        ids_buf, _ = _launch(case, M)
        assert torch.equal(ids_buf[:N], idx.cpu())
    ids, dist = _ops.vq_nearest_topm(case.z.to(_dev()), codes, e2, 3)
    assert ids.shape == (3, N) and dist.shape == (3, N) and torch.equal(ids[0], idx)


@pytest.mark.parametrize("D,K", SHAPES)
def test_a_vector_s_result_does_not_depend_on_where_it_sits(D, K):
    big, small = _case(20011, D, K, True), _case(257, D, K, True)
    take = torch.arange(1000, 1025)
    z = small.z.clone()
    z[40:65] = big.z[take]
    rows = small.allowed_row.clone()
    rows[40:65] = big.allowed_row[take]
    for M in (1, 5, 8):
        a_ids, a_dist = _launch(big, M)
        b_ids, b_dist = _launch(big, M, z=z, rows=rows)
        a_i, a_d = S.unpack(a_ids, big.ids_stride, big.N, M, S.ID_POISON, "a"), S.unpack(a_dist, big.dist_stride, big.N, M, S.DIST_POISON, "a")
        b_i, b_d = S.unpack(b_ids, 257 + 3, 257, M, S.ID_POISON, "b"), S.unpack(b_dist, 257 + 5, 257, M, S.DIST_POISON, "b")
        assert torch.equal(a_i[:, take], b_i[:, 40:65])
        assert torch.equal(a_d[:, take].view(torch.int32), b_d[:, 40:65].view(torch.int32))


@pytest.mark.parametrize("D,K", SHAPES)
def test_a_palette_of_all_codes_equals_no_palette_bit_for_bit(D, K):
    case = _case(257, D, K, True)
    everything = torch.zeros(257, dtype=torch.int64)
    for M in (1, 5, 8):
        a_ids, a_dist = _launch(case, M, rows=everything)
        b_ids, b_dist = _launch(case, M, use_palette=False)
        assert torch.equal(a_ids, b_ids) and torch.equal(a_dist.view(torch.int32), b_dist.view(torch.int32))


def test_ops_wrapper_takes_palettes_and_maps():
    from interactive_spectrogram_inpainting.vqvae import _ops
    case = _case(257, 64, 77, True)
    codes, e2 = _packed(case)
    dev = _dev()
    words = _ops.pack_palettes(case.allowed, case.K, dev)
    z = case.z.reshape(1, 257, 64).to(dev)
    ids, dist = _ops.vq_nearest_topm(z, codes, e2, 5, words, case.allowed_row.reshape(1, 257).to(dev))
    assert ids.shape == (5, 1, 257) and dist.dtype == torch.float32
    want, _ = _launch(case, 5)
    assert torch.equal(ids.reshape(5, 257).cpu(), S.unpack(want, case.ids_stride, 257, 5, S.ID_POISON, "ops"))
    with pytest.raises(ValueError):
        _ops.vq_nearest_topm(z, codes, e2, 9)
    with pytest.raises(ValueError):
        _ops.vq_nearest_topm(z, codes, e2, 2, None, case.allowed_row.reshape(1, 257))


# --------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def tiny():
    """the tiny VQVAE(in_channel=2) with calibrated codebooks of the parity tests (input [2, 2, 32, 64])"""
    from oracle import vqvae_oracle as O
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    cfg = O.Config(in_channel=2)
    sd = O.init_state_dict(cfg, seed=1)
    g = torch.Generator().manual_seed(0)
    O.calibrate_codebooks(sd, cfg, torch.randn(2, 2, 32, 64, generator=g))
    x = torch.randn(2, 2, 32, 64, generator=g)
    m = VQVAE(in_channel=2)
    m.load_state_dict(sd)
    return m.to(_dev()).eval(), x.to(_dev())


def _certify(z_nhwc, embed_dk, got, ref, what):
    """ids that differ must be near-ties of the pre-quantisation vectors (normalised float64 gap < 2e-6)"""
    bad = (got != ref).reshape(-1).nonzero().flatten().cpu()
    if bad.numel() == 0:
        return 0
    z = z_nhwc.reshape(-1, z_nhwc.shape[-1]).double().cpu()[bad]
    e = embed_dk.double().cpu()
    x2, e2 = z.pow(2).sum(1, keepdim=True), e.pow(2).sum(0)
    d = x2 - 2 * z @ e + e2
    g_, r_ = got.reshape(-1).cpu()[bad], ref.reshape(-1).cpu()[bad]
    rel = ((d.gather(1, g_[:, None]) - d.gather(1, r_[:, None])).abs() / (x2 + e2[r_][:, None])).max().item()
    assert rel < S.CERTIFY, f"{what}: an id differs from encode() and is not a near-tie ({rel:.2e})"
    return int(bad.numel())


def test_encode_topm_m1_is_encode_except_at_certified_near_ties(tiny):
    m, x = tiny
    _, _, _, id_t, id_b, _, _ = m.encode(x)
    codes_t, dist_t, codes_b, dist_b = m.encode_topm(x, m=1)
    assert codes_t.shape == (1, *id_t.shape) and codes_b.shape == (1, *id_b.shape)
    assert codes_t.dtype == torch.int64 and dist_t.dtype == torch.float32 and dist_b.shape == codes_b.shape
    enc_b = m.enc_b(x)
    z_t = m.quantize_conv_t.run(m.enc_t(enc_b), relu=False).permute(0, 2, 3, 1)
    moved_t = _certify(z_t, m.quantize_t.embed, codes_t[0], id_t, "top")
    if moved_t == 0:                                  # (the bottom level legitimately follows a moved top code)
        dec_t = m.dec_t(m.quantize_t.embed_code(id_t).permute(0, 3, 1, 2))
        z_b = m.quantize_conv_b.run(dec_t, relu=False, x2=enc_b).permute(0, 2, 3, 1)
        moved_b = _certify(z_b, m.quantize_b.embed, codes_b[0], id_b, "bottom")
        print(f"encode_topm(m=1) against encode: {moved_t} top and {moved_b} bottom ids moved at certified near-ties")


def test_render_with_palette_stays_inside_the_palettes(tiny):
    import inpainting
    import sample
    m, x = tiny
    K = m.quantize_t.n_embed
    g = torch.Generator().manual_seed(5)
    other_t, other_b = torch.randint(0, K, (1, 4, 8), generator=g), torch.randint(0, K, (1, 8, 16), generator=g)
    pal_t, pal_b = sample.codes_in_use(other_t, K), sample.codes_in_use(other_b, K)
    top, bottom = inpainting.render_with_palette(m, x, pal_t, pal_b)
    full_t, _, full_b, _ = m.encode_topm(x, m=1)
    assert top.shape == full_t.shape[1:] and bottom.shape == full_b.shape[1:] and top.dtype == torch.int64
    assert bool(pal_t[top.cpu()].all()) and bool(pal_b[bottom.cpu()].all())
    assert not torch.equal(top, full_t[0])            # 32 of 512 codes: the palette does bind
    m.decode_code(top, bottom)                        # ordinary codemaps
    everything = torch.ones(K, dtype=torch.bool)
    top_all, bottom_all = inpainting.render_with_palette(m, x, everything, everything)
    assert torch.equal(top_all, full_t[0]) and torch.equal(bottom_all, full_b[0])
    top_only, bottom_free = inpainting.render_with_palette(m, x, pal_t)
    assert torch.equal(top_only, top) and not bool(pal_b[bottom_free.cpu()].all())


def test_encode_soft_at_temperature_0_decodes_like_the_hard_codes(tiny):
    import inpainting
    m, x = tiny
    codes_t, w_t, codes_b, w_b = inpainting.encode_soft(m, x, m=4, temperature=0)
    assert codes_t.shape[0] == 4 and w_t.shape == codes_t.shape and w_b.shape == codes_b.shape
    assert bool((w_t[0] == 1).all()) and bool((w_t[1:] == 0).all())
    soft = m.decode_code_mix(codes_t, w_t, codes_b, w_b)
    hard = m.decode_code(codes_t[0], codes_b[0])
    assert torch.equal(soft.view(torch.int32), hard.view(torch.int32))
    _, w_t1, _, w_b1 = inpainting.encode_soft(m, x, m=4, temperature=0.5)
    assert bool(((w_t1.sum(0) - 1).abs() < 1e-6).all()) and bool((w_t1[:-1] >= w_t1[1:]).all())
    assert bool(((w_b1.sum(0) - 1).abs() < 1e-6).all()) and bool((w_b1[0] > 0).all())


def test_code_alternatives_are_sorted_by_distance(tiny):
    import inpainting
    m, x = tiny
    for layer in ("top", "bottom"):
        ids, dist = inpainting.code_alternatives(m, x, 8, layer)
        assert ids.shape == dist.shape and ids.shape[0] == 8 and bool((ids >= 0).all())
        assert bool((dist[:-1] <= dist[1:]).all())
    ids_t, _ = inpainting.code_alternatives(m, x, 1, "top")
    assert torch.equal(ids_t, m.encode_topm(x, m=1)[0])
