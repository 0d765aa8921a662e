"""What tests/test_vq_search_gpu.py relies on, shown without a GPU: the float64 specification of the stand-alone codebook
searches (tests_support.vq_search_spec -- the search half of the fused specification on a given z) against the oracle's
quantiser and its loss rules per route; K_max from the two LDS formulas; the case table covering every corner the kernels
have (vq_search_coverage_gaps) and every case of it free of near-ties, hand-placed rows included; the comparisons accepting
the float32 evaluation as a launch's output at every small case; and each comparison rejecting the defect it exists for --
a padding row that wins the zero vector, a half-wave merge that takes the higher of two duplicates, the two halves of a
64-row tile exchanged, the ragged tile's invalid lanes counted, counts overwritten instead of accumulated, a workgroup's
partial missing, the second pass's partial overwriting the first's, a lost row answered with code 0, and |e|^2 summed from
the wrong column."""
import collections

import pytest
import torch

import tests_support as TS

Out = collections.namedtuple("Out", "idx q counts sse_part")
CASES = TS.VQ_SEARCH_CASES


def _case(route, D, K, N, kind):
    c = TS.VqSearchCase(route, D, K, N, kind)
    assert c in CASES, TS.vq_search_case_id(c)
    return c


def _out_of(f32):
    """A launch's outputs as a correct float32 implementation would leave them: q = z + (e - z) in float32, the partials as
    the workgroups own them."""
    return Out(f32.idx.clone(), f32.z + (f32.q - f32.z), f32.counts.clone(), TS.vq_fused_partials(f32.sse_rows))


def _hold_all(out, refs, what):
    TS.vq_fused_hold_idx(out.idx, refs.spec, what)
    TS.vq_fused_hold_counts(out.counts, refs.spec, what)
    TS.vq_fused_hold_q(out.q, refs, what)
    TS.vq_fused_hold_sse(out.sse_part, refs.spec, what)


# ------------------------------------------------------------------------------------------------------------ the spec
@pytest.mark.parametrize("case", [_case(TS.VQ_EXACT, 8, 33, 257, "plain"), _case(TS.VQ_EXACT, 16, 100, 257, "plain"),
                                  _case(TS.VQ_EXACT, 32, 160, 257, "plain"), _case(TS.VQ_EXACT, 64, 96, 257, "plain"),
                                  _case(TS.VQ_F16X3, 64, 545, 257, "plain")], ids=TS.vq_search_case_id)
def test_spec_agrees_with_the_oracle(case):
    from oracle import vqvae_oracle as O
    r = TS.vq_search_case_refs(case)
    q_st, diff, ind, perplexity = O.quantize(r.z.double(), r.embed.double())
    assert torch.equal(ind, r.spec.idx) and torch.equal(r.spec.z, r.z.double())
    assert torch.allclose(q_st, r.spec.q, rtol=0, atol=1e-12)
    assert torch.allclose(diff, r.spec.diff[0], rtol=1e-12) and torch.allclose(perplexity, r.spec.perplexity[0], rtol=1e-12)
    assert int(r.spec.counts.sum()) == case.N and r.spec.counts.numel() == case.K


def test_fused_spec_is_the_search_spec_of_its_own_z():
    r = TS.vq_fused_case_refs(TS.VQ_FUSED_ROUTE_CASES[0])
    s = TS.vq_search_spec(r.spec.z, r.embed, TS.VQ_F16X3)
    for a, b in zip(s, r.spec):
        assert torch.equal(a, b)


def test_loss_rules_per_route():
    c = _case(TS.VQ_EXACT, 64, 100, 600, "lost")
    r, split = TS.vq_search_case_refs(c), TS.vq_search_case_refs(_case(TS.VQ_F16X3, 64, 100, 600, "lost"))
    assert torch.equal(r.z.view(torch.int32), split.z.view(torch.int32)) and torch.equal(r.embed, split.embed), "both routes search the same data"
    lost = torch.zeros(600, dtype=torch.bool)
    lost[list(TS.VQ_SEARCH_LOST_ROWS)] = True
    assert torch.equal(r.spec.idx < 0, lost) and int(r.spec.idx[TS.VQ_SEARCH_LOUD_ROW]) == TS.VQ_SEARCH_LOUD_CODE
    lost[TS.VQ_SEARCH_LOUD_ROW] = True                      # beyond the split-f16 pieces' range: that route alone gives it up
    s = split.spec
    assert torch.equal(s.idx < 0, lost) and torch.equal(s.idx[~lost], r.spec.idx[~lost])
    assert bool(torch.isnan(s.q[lost]).all()) and bool(torch.isnan(s.sse)) and int(s.counts.sum()) == 596
    part = TS.vq_fused_partials(s.sse_rows)
    assert torch.isnan(part).tolist() == [True, False, True], "workgroup 1 owns no lost row"
    # a non-finite code: the split-f16 route gives every vector up; on the exact route the code is absent
    b = TS.vq_search_case_refs(_case(TS.VQ_EXACT, 64, 100, 257, "badcode"))
    bad = sorted(k % 100 for k in TS.VQ_SEARCH_BAD_CODES)
    assert (~torch.isfinite(b.embed).all(dim=0)).nonzero().reshape(-1).tolist() == bad
    assert bool((TS.vq_search_spec(b.z, b.embed, TS.VQ_F16X3).idx == -1).all())
    keep = torch.isfinite(b.embed).all(dim=0)
    without = TS.vq_search_spec(b.z, b.embed[:, keep], TS.VQ_EXACT)
    assert torch.equal(keep.nonzero().reshape(-1)[without.idx], b.spec.idx) and torch.equal(without.q, b.spec.q)
    assert not bool(torch.isin(b.spec.idx, torch.tensor(bad)).any()) and int(b.spec.counts.sum()) == 257
    assert bool((TS.vq_search_spec(b.z, torch.full((64, 3), float("nan")), TS.VQ_EXACT).idx == -1).all())


def test_k_max_follows_the_lds_formulas():
    assert [TS.vq_search_k_max(D) for D in TS.VQ_SEARCH_DIMS] == [2720, 1728, 992, 544] and TS.vq_search_k_max(64, True) == 576
    for D in TS.VQ_SEARCH_DIMS:
        K = TS.vq_search_k_max(D)
        assert (K * (D + 4) + 2 * K + 8) * 4 <= 150 * 1024 < ((K + 32) * (D + 4) + 2 * (K + 32) + 8) * 4
    assert TS.vq_search_lds_bytes(64, 576, True) == 576 * 264 + 576 // 8 + 48 <= 150 * 1024 < TS.vq_search_lds_bytes(64, 608, True)


# -------------------------------------------------------------------------------------------------------- the case data
def test_table_covers_every_corner():
    assert TS.vq_search_coverage_gaps(CASES) == []
    assert len(set(CASES)) == len(CASES)
    ids = {TS.vq_search_case_id(c) for c in CASES}
    for want in ("exact-D8-K2720-N257-plain", "exact-D16-K1728-N257-plain", "exact-D32-K992-N257-plain", "exact-D64-K544-N257-plain",
                 "f16x3-D64-K576-N257-plain", "f16x3-D64-K545-N257-plain", "exact-D32-K96-N257-plain", "exact-D32-K160-N257-plain",
                 "f16x3-D64-K96-N257-plain", "f16x3-D64-K160-N257-plain", "f16x3-D64-K5-N257-far_all",
                 "exact-D8-K33-N65793-plain", "f16x3-D64-K96-N65793-plain"):
        assert want in ids, want
    # ... and the assertion notices a corner that is dropped
    def without(pred):
        return TS.vq_search_coverage_gaps([c for c in CASES if not pred(c)])
    assert any("exact D=32" in g for g in without(lambda c: c.D == 32))
    assert without(lambda c: c.route == TS.VQ_F16X3 and c.K in (96, 160)) and without(lambda c: c.D == 16 and c.K == 96)
    assert without(lambda c: c.K == TS.vq_search_k_max(c.D, c.route == TS.VQ_F16X3))
    assert without(lambda c: c.kind == "far_all") and without(lambda c: c.N > 65536 and c.route == TS.VQ_EXACT)
    assert without(lambda c: c.N == 32) and without(lambda c: c.N == 256) and without(lambda c: c.kind == "lost" and c.D == 8)


@pytest.mark.parametrize("case", CASES, ids=TS.vq_search_case_id)
def test_case_data_has_no_near_tie(case):
    r = TS.vq_search_case_refs(case)
    live = r.spec.idx >= 0
    assert r.z.shape == (case.N, case.D) and r.embed.shape == (case.D, case.K) and r.z.dtype == r.embed.dtype == torch.float32
    gaps = TS.vq_search_gaps(r.z, r.embed, r.alias)
    if bool(live.any()):
        assert float(gaps[live].min()) >= TS.VQ_FUSED_MIN_GAP, "hand-placed rows included"
    assert torch.equal(r.f32.idx, r.spec.idx), "a float32 evaluation of the whole formula returns the spec's indices"
    assert torch.equal(live, ~TS.vq_search_lost(r.z, r.embed, case.route))
    if case.kind not in ("lost", "badcode"):
        assert bool(live.all())


def test_hand_placed_rows_are_where_the_cases_say():
    for route, D in TS.VQ_SEARCH_ROUTES:
        r = TS.vq_search_case_refs(_case(route, D, 100, 257, "edges"))
        rows = TS.VQ_SEARCH_EDGE_ROWS
        assert int(r.spec.idx[rows["code"]]) == 50 and TS.same_bits(r.z[rows["code"]], r.embed[:, 50])
        nearest_origin = int(r.embed.double().pow(2).sum(dim=0).argmin())
        assert not bool(r.z[rows["zero"]].any()) and int(r.spec.idx[rows["zero"]]) == nearest_origin
        assert abs(float(r.z[rows["tiny"]].double().norm()) - 1e-3) < 1e-9 and int(r.spec.idx[rows["tiny"]]) == nearest_origin
        assert int(r.frozen.sum()) == 3
        for K in (96,) + ((64, 512) if D == 64 else ()):
            r = TS.vq_search_case_refs(_case(route, D, K, 257, "dups"))
            sources, copies = TS.vq_search_dup_layout(K)
            for src, (same_tile, other_tile), row in zip(sources, copies, TS.VQ_SEARCH_DUP_ROWS):
                assert same_tile // 32 == src // 32 and (same_tile & 4) != (src & 4) and other_tile // 32 != src // 32
                assert all(c > src and torch.equal(r.embed[:, c], r.embed[:, src]) and int(r.alias[c]) == src for c in (same_tile, other_tile))
                assert TS.same_bits(r.z[row], r.embed[:, src]) and int(r.spec.idx[row]) == src, "the lowest index wins"
                assert int(r.spec.counts[same_tile]) == 0 and int(r.spec.counts[other_tile]) == 0
            raw = TS.vq_search_gaps(r.z, r.embed)
            assert bool((raw[list(TS.VQ_SEARCH_DUP_ROWS[:len(sources)])] == 0).all())
    assert TS.vq_search_dup_layout(512) == (TS.VQ_FUSED_DUP_SOURCES, TS.VQ_FUSED_DUP_COPIES)
    for kind, rows in TS.VQ_SEARCH_FAR_ROWS.items():
        c = [c for c in CASES if c.kind == kind][0]
        r = TS.vq_search_case_refs(c)
        for row, code in rows.items():
            assert int(r.spec.idx[row]) == code and float(r.embed[:, code].abs().max()) >= 64.0 and bool(r.frozen[row])
    far = lambda r: r.embed.abs().amax(dim=0) >= 64.0
    r = TS.vq_search_case_refs(_case(TS.VQ_F16X3, 64, 512, 257, "far_scan"))
    assert int(far(r).sum()) == 42 and int(r.spec.counts[far(r)].sum()) == 2
    r = TS.vq_search_case_refs(_case(TS.VQ_F16X3, 64, 100, 257, "far_pad"))
    assert far(r).nonzero().reshape(-1).tolist() == [98, 99], "both in the padded last tile"
    r = TS.vq_search_case_refs(_case(TS.VQ_F16X3, 64, 5, 257, "far_all"))
    assert bool(far(r).all())
    r = TS.vq_search_case_refs(_case(TS.VQ_F16X3, 64, 160, 257, "far_certified"))
    assert int(far(r).sum()) == 10
    # the certificate of vq_decide_f32, in float64 with a tenth of its room: (min |e_far| - |z|)^2 > the winner's distance
    n_far = r.embed[:, far(r)].double().norm(dim=0).min()
    assert bool(((n_far - r.z.double().norm(dim=1)).pow(2) * 0.9 > r.spec.sse_rows).all()) and int(r.spec.counts[far(r)].sum()) == 0


# --------------------------------------------------------------------------------------------------------- acceptance
def test_comparisons_accept_the_float32_evaluation():
    for case in CASES:
        if case.N < 1000:
            r = TS.vq_search_case_refs(case)
            _hold_all(_out_of(r.f32), r, TS.vq_search_case_id(case))


def test_pack_codebook_yardstick_accepts_itself():
    g = torch.Generator().manual_seed(5)
    for D in TS.VQ_SEARCH_DIMS:
        embed = torch.randn(D, 257, generator=g)
        codes, e2 = TS.vq_pack_codebook_spec(embed)
        assert codes.shape == (257, D) and TS.same_bits(codes[100], embed[:, 100]) and e2.shape == (257, 1)
        yard = TS.vq_pack_codebook_f32(embed)
        assert TS.compare_rows(yard, e2, yard, f"e2 D={D}").ratio <= 1.0
        assert TS.row_error(yard, e2) <= D * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- defects
EDGES = _case(TS.VQ_EXACT, 32, 100, 257, "edges")
SECOND = _case(TS.VQ_EXACT, 8, 33, TS.VQ_SEARCH_SECOND_PASS_N, "plain")


def test_rejects_a_padding_row_that_wins_the_origin():
    r = TS.vq_search_case_refs(EDGES)
    padded = torch.cat([r.embed, torch.zeros(32, 128 - 100)], dim=1)         # padding rows with |e|^2 = 0 in place of +inf
    bad = TS.vq_search_f32(r.z, padded)
    for row in (TS.VQ_SEARCH_EDGE_ROWS["zero"], TS.VQ_SEARCH_EDGE_ROWS["tiny"]):
        assert int(bad.idx[row]) >= 100
    with pytest.raises(AssertionError, match="indices differ"):
        TS.vq_fused_hold_idx(bad.idx, r.spec, "padding")
    idx = r.spec.idx.clone()
    idx[TS.VQ_SEARCH_EDGE_ROWS["zero"]] = 0                                  # ... or clamped into the codebook
    with pytest.raises(AssertionError, match="indices differ"):
        TS.vq_fused_hold_idx(idx, r.spec, "padding")
    with pytest.raises(AssertionError, match="counts differ"):
        TS.vq_fused_hold_counts(torch.bincount(idx, minlength=100), r.spec, "padding")


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "dups"], ids=TS.vq_search_case_id)
def test_rejects_a_merge_that_takes_the_higher_duplicate(case):
    r = TS.vq_search_case_refs(case)
    sources, copies = TS.vq_search_dup_layout(case.K)
    for which in (0, 1):                                   # the other lane half of the same tile; another tile
        idx = r.spec.idx.clone()
        for src, cs in zip(sources, copies):
            idx[idx == src] = cs[which]
        with pytest.raises(AssertionError, match="indices differ"):
            TS.vq_fused_hold_idx(idx, r.spec, "tie")
        with pytest.raises(AssertionError, match="counts differ"):
            TS.vq_fused_hold_counts(torch.bincount(idx, minlength=case.K), r.spec, "tie")


def test_rejects_exchanged_halves_of_a_tile():
    r = TS.vq_search_case_refs(EDGES)
    good = _out_of(r.f32)
    idx, q = good.idx.clone(), good.q.clone()
    for t in (idx, q):
        t[64:96], t[96:128] = t[96:128].clone(), t[64:96].clone()
    TS.vq_fused_hold_counts(good.counts, r.spec, "halves")                   # (the histogram cannot tell)
    with pytest.raises(AssertionError, match="indices differ"):
        TS.vq_fused_hold_idx(idx, r.spec, "halves")
    with pytest.raises(AssertionError, match="one float32 ulp"):
        TS.vq_fused_hold_q(q, r, "halves")


def test_rejects_counted_invalid_lanes():
    r = TS.vq_search_case_refs(EDGES)
    counts = r.spec.counts.clone()
    counts[r.spec.idx[TS.VQ_SEARCH_EDGE_ROWS["zero"]]] += 256 - 257 % 256    # the ragged tile's idle lanes hold zero vectors
    with pytest.raises(AssertionError, match="counts differ"):
        TS.vq_fused_hold_counts(counts, r.spec, "idle lanes")


def test_rejects_overwritten_counts():
    r = TS.vq_search_case_refs(EDGES)
    start = torch.arange(100) % 7
    TS.vq_fused_hold_counts((start + r.spec.counts) - start, r.spec, "accumulated")
    with pytest.raises(AssertionError, match="counts differ"):
        TS.vq_fused_hold_counts(r.spec.counts - start, r.spec, "overwritten")


def test_rejects_a_missing_or_overwritten_partial():
    r = TS.vq_search_case_refs(SECOND)
    N = SECOND.N
    good = TS.vq_fused_partials(r.f32.sse_rows)
    assert good.numel() == 256 and -(-N // 256) == 258
    TS.vq_fused_hold_sse(good, r.spec, "partials")
    for g in (0, 1, 255):
        part = good.clone()
        part[g] = float("nan")                             # never written
        with pytest.raises(AssertionError, match="were not written"):
            TS.vq_fused_hold_sse(part, r.spec, "partials")
        part[g] = 0.0                                      # written without the workgroup's sum
        with pytest.raises(AssertionError, match="summed squared error"):
            TS.vq_fused_hold_sse(part, r.spec, "partials")
    second = torch.where(torch.arange(N) >= 65536, r.f32.sse_rows, torch.zeros(()))
    part = good.clone()
    part[:2] = TS.vq_fused_partials(second)[:2]            # the second pass's sum in place of first + second
    with pytest.raises(AssertionError, match="summed squared error"):
        TS.vq_fused_hold_sse(part, r.spec, "partials")
    with pytest.raises(AssertionError, match="partials"):
        TS.vq_fused_hold_sse(good[:255], r.spec, "partials")


def test_rejects_a_lost_row_answered_with_code_0():
    c = _case(TS.VQ_EXACT, 16, 100, 600, "lost")
    r = TS.vq_search_case_refs(c)
    good = _out_of(r.f32)
    _hold_all(good, r, "lost")
    lost = r.spec.idx < 0
    idx, q, counts = good.idx.clone(), good.q.clone(), good.counts.clone()
    idx[lost], q[lost] = 0, r.embed[:, 0]
    counts[0] += int(lost.sum())
    with pytest.raises(AssertionError, match="indices differ"):
        TS.vq_fused_hold_idx(idx, r.spec, "lost")
    with pytest.raises(AssertionError, match="counts differ"):
        TS.vq_fused_hold_counts(counts, r.spec, "lost")
    with pytest.raises(AssertionError, match="is not NaN"):
        TS.vq_fused_hold_q(q, r, "lost")
    with pytest.raises(AssertionError, match="not NaN"):
        TS.vq_fused_hold_sse(torch.nan_to_num(good.sse_part, nan=0.0), r.spec, "lost")


@pytest.mark.parametrize("D", TS.VQ_SEARCH_DIMS)
def test_rejects_e2_summed_from_the_wrong_column(D):
    embed = torch.randn(D, 257, generator=torch.Generator().manual_seed(D))
    _, e2 = TS.vq_pack_codebook_spec(embed)
    with pytest.raises(AssertionError, match="times the float32 yardstick"):
        TS.compare_rows(TS.vq_pack_codebook_f32(embed, exchanged=True), e2, TS.vq_pack_codebook_f32(embed), "e2")
