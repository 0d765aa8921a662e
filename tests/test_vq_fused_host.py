"""What tests/test_vq_fused_gpu.py relies on, shown without a GPU: the float64 specification of the fused quantize_conv +
codebook search (tests_support.vq_fused_spec) against the oracle's quantiser applied to the spec's z; the case data of every
case in the table free of near-ties (gap >= VQ_FUSED_MIN_GAP); the comparisons accepting the float32 evaluation as a launch's
output at every small case; and each comparison rejecting the defect it is meant for -- a tile's rows shifted by one, the
second source's chunk read from the first, the ragged last tile left unwritten, a padded codebook row allowed to win, a tie
resolved to the higher index, counts accumulated onto stale contents, one workgroup's partial missing."""
import collections

import pytest
import torch

import tests_support as TS

Out = collections.namedtuple("Out", "idx q q_pair z counts sse_part")
SENTINEL = -7777


def _k_max():
    from interactive_spectrogram_inpainting import _hip
    return TS.vq_fused_k_max(_hip.lib())


def _small_cases():
    cases = TS.VQ_FUSED_ROUTE_CASES + TS.VQ_FUSED_PIXEL_CASES + TS.vq_fused_k_cases(_k_max()) + TS.VQ_FUSED_STRIDED_CASES
    return [c for c in dict.fromkeys(cases) if c.B * c.H * c.W < 1000]


def _out_of(f32):
    """A launch's outputs as a correct float32 implementation would leave them: the float32 evaluation's z and indices,
    q = z + (e - z) in float32, its pair copy, the histogram, and the partials as the workgroups own them."""
    live = f32.idx >= 0
    q = f32.z + (f32.q - f32.z)
    q_pair = torch.full_like(q, float("nan"))
    q_pair[live] = TS.pair_encode_host(q[live])
    return Out(f32.idx.clone(), q, q_pair, f32.z.clone(), f32.counts.clone(), TS.vq_fused_partials(f32.sse_rows))


def _hold_all(out, refs, what):
    TS.vq_fused_hold_idx(out.idx, refs.spec, what)
    TS.vq_fused_hold_counts(out.counts, refs.spec, what)
    TS.vq_fused_hold_z(out.z, refs, what)
    TS.vq_fused_hold_q(out.q, refs, what)
    TS.vq_fused_hold_q_pair(out.q_pair, out.q, refs, what)
    TS.vq_fused_hold_sse(out.sse_part, refs.spec, what)


ROUTE = TS.VQ_FUSED_ROUTE_CASES[6]                        # (64, 128), K = 512, N = 257: the models' bottom level
assert (ROUTE.C0, ROUTE.C1) == (64, 128)


# ------------------------------------------------------------------------------------------------------------ the spec
@pytest.mark.parametrize("case", [TS.VQ_FUSED_ROUTE_CASES[0], ROUTE, TS.VQ_FUSED_PIXEL_CASES[9], TS.VqFusedCase(64, 0, 40, 1, 1, 257, False)],
                         ids=TS.vq_fused_case_id)
def test_spec_agrees_with_the_oracle_on_its_own_z(case):
    from oracle import vqvae_oracle as O
    r = TS.vq_fused_case_refs(case)
    q_st, diff, ind, perplexity = O.quantize(r.spec.z, r.embed.double())
    assert torch.equal(ind, r.spec.idx)
    assert torch.allclose(q_st, r.spec.q, rtol=0, atol=1e-12)            # (z + (e - z) in float64)
    assert torch.allclose(diff, r.spec.diff[0], rtol=1e-12) and torch.allclose(perplexity, r.spec.perplexity[0], rtol=1e-12)
    assert int(r.spec.counts.sum()) == r.spec.idx.numel() and r.spec.counts.numel() == case.K
    a = r.a0 if r.a1 is None else torch.cat([r.a0, r.a1], dim=1)
    assert torch.equal(TS.pair_round_f16(a), a) and bool((a >= 0).all()), "rectified, and exact in the pair format"
    assert torch.equal(TS.pair_decode_host(TS.pair_encode_host(a)), a)


def test_spec_is_loud_about_non_finite_operands():
    r = TS.vq_fused_case_refs(ROUTE)
    a0, a1 = r.a0.clone(), r.a1.clone()
    a0[5, 3], a1[200, 77], a0[9, 60] = float("nan"), float("inf"), 3.0e4
    s = TS.vq_fused_spec(a0, a1, r.W, r.bias, r.embed)
    lost = torch.zeros(257, dtype=torch.bool)
    lost[[5, 9, 200]] = True
    assert torch.equal(s.idx < 0, lost) and torch.equal(s.idx[~lost], r.spec.idx[~lost])
    assert bool(torch.isnan(s.q[lost]).all()) and torch.equal(s.q[~lost], r.spec.q[~lost])
    assert bool(torch.isnan(s.sse)) and bool(torch.isnan(s.diff).all()) and int(s.counts.sum()) == 254
    bad = r.embed.clone()
    bad[3, 100] = float("inf")
    s = TS.vq_fused_spec(r.a0, r.a1, r.W, r.bias, bad)
    assert bool((s.idx == -1).all()) and bool(torch.isnan(s.q).all()) and bool(torch.isnan(s.sse)) and int(s.counts.sum()) == 0


# -------------------------------------------------------------------------------------------------------- the case data
def _all_cases():
    cases = TS.VQ_FUSED_ROUTE_CASES + TS.VQ_FUSED_PIXEL_CASES + TS.vq_fused_k_cases(576) + TS.VQ_FUSED_STRIDED_CASES
    return list(dict.fromkeys(cases))


@pytest.mark.parametrize("case", _all_cases(), ids=TS.vq_fused_case_id)
def test_case_data_has_no_near_tie(case):
    r = TS.vq_fused_case_refs(case)
    gaps = TS.vq_fused_gaps(r.spec.z, r.embed)
    assert gaps.shape == (case.B * case.H * case.W,) and float(gaps.min()) >= TS.VQ_FUSED_MIN_GAP
    assert torch.equal(r.f32.idx, r.spec.idx), "a float32 evaluation of the whole formula returns the spec's indices"
    if case.B * case.H * case.W >= 2 * case.K:
        assert bool((r.spec.counts > 0).all()), "every code is used"


def test_k_max_is_what_the_table_assumes():
    assert _k_max() == 576, "test_case_data_has_no_near_tie covers the K_max case at this K"


def test_duplicate_codes_tie_exactly_and_only_with_their_copies():
    r = TS.vq_fused_case_refs(ROUTE, dups=True)
    e = r.embed
    for src, copies in zip(TS.VQ_FUSED_DUP_SOURCES, TS.VQ_FUSED_DUP_COPIES):
        same_tile, other_tile = copies
        assert same_tile // 32 == src // 32 and (same_tile & 4) != (src & 4) and other_tile // 32 != src // 32
        assert all(c > src and torch.equal(e[:, c], e[:, src]) and int(r.alias[c]) == src for c in copies)
        assert int(r.spec.counts[src]) >= 1 and all(int(r.spec.counts[c]) == 0 for c in copies), "the lowest index wins"
    tied = torch.isin(r.spec.idx, torch.tensor(TS.VQ_FUSED_DUP_SOURCES))
    gaps, raw = TS.vq_fused_gaps(r.spec.z, r.embed, r.alias), TS.vq_fused_gaps(r.spec.z, r.embed)
    assert float(gaps.min()) >= TS.VQ_FUSED_MIN_GAP and bool((raw[tied] == 0).all()) and torch.equal(raw[~tied], gaps[~tied])


def test_far_code_case_places_its_pixels():
    data = TS.vq_fused_far_case_data(ROUTE)
    r = TS.vq_fused_refs(*data)
    gaps = TS.vq_fused_gaps(r.spec.z, r.embed)
    assert float(gaps.min()) >= TS.VQ_FUSED_MIN_GAP and torch.equal(r.f32.idx, r.spec.idx)
    for pixel, code in TS.VQ_FUSED_FAR_PIXELS.items():
        assert int(r.spec.idx[pixel]) == code and float(r.embed[:, code].abs().max()) >= 64.0
    far = r.embed.abs().amax(dim=0) >= 64.0
    assert int(far.sum()) == 42 and int(r.spec.counts[far].sum()) == 2, "40 dead codes, the scaled neighbour, code 200; two win"
    assert torch.equal(r.spec.z.float(), torch.cat([r.a0, r.a1], dim=1)[:, 32:96]), "the identity block hands the activations on"
    _hold_all(_out_of(r.f32), r, "far codes")


# --------------------------------------------------------------------------------------------------------- acceptance
def test_comparisons_accept_the_float32_evaluation():
    for case in _small_cases():
        r = TS.vq_fused_case_refs(case)
        _hold_all(_out_of(r.f32), r, TS.vq_fused_case_id(case))
    r = TS.vq_fused_case_refs(ROUTE, dups=True)
    _hold_all(_out_of(r.f32), r, "duplicates")


def test_partials_follow_the_grid():
    assert [TS.vq_num_partials(n) for n in (1, 256, 257, 65536, 65537, 66603)] == [1, 1, 2, 256, 256, 256]
    rows = torch.arange(66603, dtype=torch.float64)
    part = TS.vq_fused_partials(rows)
    assert part.shape == (256,) and float(part.sum()) == float(rows.sum())
    assert float(part[0]) == float(rows[:256].sum() + rows[65536:65792].sum())          # workgroup 0's second pass
    assert float(part[4]) == float(rows[1024:1280].sum() + rows[66560:].sum())          # the ragged tile 260 is workgroup 4's
    assert float(part[5]) == float(rows[1280:1536].sum())


# ------------------------------------------------------------------------------------------------------------- defects
BIG = TS.VQ_FUSED_PIXEL_CASES[-1]                          # (32, 0), K = 64, N = 66 603: two passes and a ragged tile
assert BIG.B * BIG.H * BIG.W == 66603


def test_rejects_a_tile_shifted_by_one_row():
    r = TS.vq_fused_case_refs(BIG)
    good = _out_of(r.f32)
    tile = slice(65536 + 256, 65536 + 512)                # workgroup 1's second pass
    idx, q, z = good.idx.clone(), good.q.clone(), good.z.clone()
    for t in (idx, q, z):
        t[tile] = torch.roll(t[tile], 1, dims=0)
    bad = good._replace(idx=idx, q=q, z=z, counts=good.counts)       # (the histogram of a shifted tile is unchanged)
    TS.vq_fused_hold_counts(bad.counts, r.spec, "shift")
    with pytest.raises(AssertionError, match="indices differ"):
        TS.vq_fused_hold_idx(bad.idx, r.spec, "shift")
    assert int((idx != r.spec.idx).sum()) <= 256 < 0.01 * idx.numel(), "within the 1 % the whole-model tests allow"
    with pytest.raises(AssertionError, match="times the float32 yardstick"):
        TS.vq_fused_hold_z(bad.z, r, "shift")
    with pytest.raises(AssertionError, match="one float32 ulp"):
        TS.vq_fused_hold_q(bad.q, r, "shift")


def test_rejects_the_second_source_read_from_the_first():
    r = TS.vq_fused_case_refs(ROUTE)
    a1 = r.a1.clone()
    a1[:, :32] = r.a0[:, :32]                             # the second source's first chunk comes from the first source
    bad = _out_of(TS.vq_fused_f32(r.a0, a1, r.W, r.bias, r.embed))
    with pytest.raises(AssertionError, match="times the float32 yardstick"):
        TS.vq_fused_hold_z(bad.z, r, "chunk")
    with pytest.raises(AssertionError, match="indices differ"):
        TS.vq_fused_hold_idx(bad.idx, r.spec, "chunk")


def test_rejects_an_unwritten_ragged_tile():
    r = TS.vq_fused_case_refs(ROUTE)                      # N = 257: the last tile holds one pixel
    good = _out_of(r.f32)
    idx, q, z, q_pair, counts = good.idx.clone(), good.q.clone(), good.z.clone(), good.q_pair.clone(), good.counts.clone()
    idx[256], q[256], z[256], q_pair[256] = SENTINEL, float("nan"), float("nan"), float("nan")
    counts[good.idx[256]] -= 1
    part = good.sse_part.clone()
    part[1] = float("nan")
    with pytest.raises(AssertionError, match="indices differ"):
        TS.vq_fused_hold_idx(idx, r.spec, "ragged")
    with pytest.raises(AssertionError, match="counts differ"):
        TS.vq_fused_hold_counts(counts, r.spec, "ragged")
    with pytest.raises(AssertionError, match="yardstick"):
        TS.vq_fused_hold_z(z, r, "ragged")
    with pytest.raises(AssertionError, match="not finite"):
        TS.vq_fused_hold_q(q, r, "ragged")
    with pytest.raises(AssertionError, match="from q"):
        TS.vq_fused_hold_q_pair(q_pair, good.q, r, "ragged")
    with pytest.raises(AssertionError, match="were not written"):
        TS.vq_fused_hold_sse(part, r.spec, "ragged")


@pytest.mark.parametrize("K", [16, 40, 500])
def test_rejects_a_padded_codebook_row_that_wins(K):
    case = TS.vq_fused_k_cases(576)[TS.VQ_FUSED_K_SIZES.index(K)]
    r = TS.vq_fused_case_refs(case)
    Kp = (K + 31) // 32 * 32
    # the LDS image's padding rows are zero vectors: the defect gives them |e|^2 = 0 where the kernel gives them 2^100 (the
    # origin is nearer to many a pixel than its code is: |z|^2 is about 32, two pixels are about 64 apart)
    padded = torch.cat([r.embed, torch.zeros(TS.VQ_FUSED_D, Kp - K)], dim=1)
    bad = _out_of(TS.vq_fused_f32(r.a0, r.a1, r.W, r.bias, padded))
    wrong = bad.idx >= K
    assert bool(wrong.any()), "no pixel of this case lies nearer the origin than any code: the defect would not show"
    with pytest.raises(AssertionError, match="indices differ"):
        TS.vq_fused_hold_idx(bad.idx, r.spec, "padding")
    with pytest.raises(AssertionError, match="counts differ"):
        TS.vq_fused_hold_counts(bad.counts, r.spec, "padding")


def test_rejects_a_tie_resolved_to_the_higher_index():
    r = TS.vq_fused_case_refs(ROUTE, dups=True)
    good = _out_of(r.f32)
    for which in (0, 1):                                  # the copy in the same tile's other lane half; the one in another tile
        idx = good.idx.clone()
        for src, copies in zip(TS.VQ_FUSED_DUP_SOURCES, TS.VQ_FUSED_DUP_COPIES):
            idx[idx == src] = copies[which]
        counts = torch.bincount(idx, minlength=ROUTE.K)
        with pytest.raises(AssertionError, match="indices differ"):
            TS.vq_fused_hold_idx(idx, r.spec, "tie")
        with pytest.raises(AssertionError, match="counts differ"):
            TS.vq_fused_hold_counts(counts, r.spec, "tie")
        TS.vq_fused_hold_q(good.q, r, "tie")              # (q cannot tell: the copies are the same vector)


def test_rejects_counts_on_top_of_stale_contents():
    r = TS.vq_fused_case_refs(ROUTE)
    stale = torch.zeros(ROUTE.K, dtype=torch.int64)
    stale[500] = 1
    with pytest.raises(AssertionError, match="counts differ"):
        TS.vq_fused_hold_counts(r.spec.counts + stale, r.spec, "stale")
    with pytest.raises(AssertionError, match="counts differ"):
        TS.vq_fused_hold_counts(r.spec.counts * 2, r.spec, "stale")


def test_rejects_a_missing_partial():
    r = TS.vq_fused_case_refs(BIG)
    good = TS.vq_fused_partials(r.f32.sse_rows)
    TS.vq_fused_hold_sse(good, r.spec, "partials")
    for g in (0, 4, 255):
        part = good.clone()
        part[g] = 0.0                                     # written, but without the workgroup's sum: 1 / 256 of the total
        with pytest.raises(AssertionError, match="summed squared error"):
            TS.vq_fused_hold_sse(part, r.spec, "partials")
        part[g] = float("nan")                            # never written
        with pytest.raises(AssertionError, match="were not written"):
            TS.vq_fused_hold_sse(part, r.spec, "partials")
    part = good.clone()
    part[0] -= float(TS.vq_fused_partials(torch.where(torch.arange(66603) < 65536, 0.0, 1.0) * r.f32.sse_rows.double())[0])
    with pytest.raises(AssertionError, match="summed squared error"):                    # workgroup 0's second pass alone
        TS.vq_fused_hold_sse(part, r.spec, "partials")
    with pytest.raises(AssertionError, match="partials"):
        TS.vq_fused_hold_sse(good[:255], r.spec, "partials")
