"""The float64 specification of the relative-attention forward (tests/tests_support.py), held on the host: against
oracle/prior_oracle.py, against its own definitions, and against mutants -- what the hold of
tests/test_attention_fwd_gpu.py rejects.  The route restatement is held to the committed launch trace
(tests/attention_plan_trace.txt), the case table to its requirements.  No GPU, no compiler."""
import math
import pathlib

import pytest
import torch

import tests_support as T
from test_attention_plan_host import (EXPECTED, F_B, F_CUS, F_DENSE, F_ENTRY, F_EVENTS, F_H, F_HD, F_KNOBS, F_LEN, F_MASK, F_PREC, F_TABLE,
                                      F_WS)

HOST_CUS = 8          # persistent cases are resolved for a small device here: the same schedules at a fraction of the pairs
CASES = T.ATTENTION_FWD_CASES
IDS = [T.attention_fwd_case_id(c) for c in CASES]


def _refs(c):
    return T.attention_fwd_case_refs(c, HOST_CUS)


def _args(c, d):
    return (d.q, d.k, d.v, d.rel, c.H, c.Cq, c.Ck, d.Ek, c.mask, d.dense, d.scale)


def _gather_formula(q, k, v, rel, H, Cq, Ck, Ek, mask, scale):
    """The formula of tests/test_prior_gpu.py::test_rel_attention_against_spec, in float64."""
    from oracle import prior_oracle as P
    hq, hk, hv = (t.double().permute(1, 2, 0, 3) for t in (q, k, v))
    B, _, Sq, _ = hq.shape
    Sk = hk.shape[2]
    logits = hq @ hk.transpose(-1, -2)
    if rel is not None:
        qe = torch.einsum("bhid,hrd->bhir", hq, rel.double())
        logits = logits + qe.gather(3, P.rel_index(Sq, Sk, Cq, Ck, Ek).expand(B, H, Sq, Sk))
    logits = logits * scale
    if mask is not None:
        logits = logits + mask
    return torch.softmax(logits, -1) @ hv, torch.logsumexp(logits, -1), logits


def _mask(mode, Sq, Sk):
    i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    if mode == 0:
        return None
    return torch.zeros(Sq, Sk, dtype=torch.float64).masked_fill((j > i) if mode == 1 else (j < i), float("-inf"))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("table", [True, False])
def test_spec_equals_the_oracle_on_self_attention(mode, table):
    """oracle/prior_oracle.py::attention with identity projections (self-attention, the mask as a dense tensor)."""
    from oracle import prior_oracle as P
    torch.manual_seed(3 + mode)
    S, B, H, hd, C = 40, 2, 3, 16, 4
    d, E = H * hd, S // C
    x = torch.randn(S, B, d, dtype=torch.float64)
    rel = torch.randn(H, 2 * E - 1, hd, dtype=torch.float64)
    eye = torch.eye(d, dtype=torch.float64)
    sd = {"in_proj_weight": torch.cat([eye, eye, eye]), "in_proj_bias": torch.zeros(3 * d, dtype=torch.float64), "out_proj.weight": eye,
          "out_proj.bias": torch.zeros(d, dtype=torch.float64), "rel_embeddings": rel}
    want = P.attention(x, x, sd, "", H, C, E, C, E, _mask(mode, S, S), bias=table)
    got = T.attention_fwd_spec(x, x, x, rel if table else None, H, C, C, E, mode, None, 1.0 / math.sqrt(hd))
    assert float((got.out.permute(2, 0, 1, 3).reshape(S, B, d) - want).abs().max()) < 1e-12


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("Sq,Sk,Cq,Ck,ek_extra,table", [(33, 50, 1, 1, 0, True), (40, 17, 4, 1, 0, True), (17, 40, 1, 4, 2, True), (50, 33, 3, 2, 0, True),
                                                        (33, 50, 2, 1, 0, False)])
def test_spec_equals_the_gather_formula(mode, Sq, Sk, Cq, Ck, ek_extra, table):
    """Cross-attention and several channels per event: the `rel_index` gather formula of the existing tests, in float64;
    out, lse and the kept logits.  (Anti-causal rows beyond the last key are left out: softmax has no answer there.)"""
    torch.manual_seed(Sq + Sk + mode)
    B, H, hd = 2, 2, 16
    q, k, v = torch.randn(Sq, B, H, hd), torch.randn(Sk, B, H, hd), torch.randn(Sk, B, H, hd)
    Ek = -(-Sk // Ck) + ek_extra
    rel = torch.randn(H, -(-Sq // Cq) + Ek - 1, hd) if table else None
    scale = 0.2
    out, lse, logits = _gather_formula(q, k, v, rel, H, Cq, Ck, Ek, _mask(mode, Sq, Sk), scale)
    got = T.attention_fwd_spec(q, k, v, rel, H, Cq, Ck, Ek, mode, None, scale)
    rows = slice(0, min(Sq, Sk) if mode == 2 else Sq)
    assert float((got.out[:, :, rows] - out[:, :, rows]).abs().max()) < 1e-12
    assert float((got.lse[:, :, rows] - lse[:, :, rows]).abs().max()) < 1e-12
    fin = got.allowed.expand_as(logits)
    assert float((got.logits2[fin] - logits[fin] * T.ATTN_LOG2E).abs().max()) < 1e-12
    if mode == 2 and Sq > Sk:
        assert bool((got.lse[:, :, Sk:] == T.ATTN_EMPTY_LSE).all()) and bool((got.out[:, :, Sk:] == 0).all())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_is_consistent_and_the_yardsticks_pass_the_hold(c):
    """out = softmax(ln2 logits2) v and lse = logsumexp(ln2 logits2) on the spec's own logits; the empty rows are exactly the
    rows the case data designs; the float32 yardstick is finite (attention_fwd_refs asserts it), the f16 model in range
    (attention_fwd_model asserts it); the unmutated yardstick and the mode's model pass the hold against the spec."""
    r, d, refs = _refs(c)
    spec = refs.spec
    nat = torch.where(spec.allowed, spec.logits2, torch.full_like(spec.logits2, float("-inf"))) * math.log(2.0)
    live = ~refs.empty
    hv = d.v.double().permute(1, 2, 0, 3)
    assert float(((torch.softmax(nat, -1) @ hv)[live] - spec.out[live]).abs().max()) < 1e-11 if bool(live.any()) else True
    assert float((torch.logsumexp(nat, -1)[live] - spec.lse[live]).abs().max()) < 1e-10 if bool(live.any()) else True
    empty_rows = sorted(set(torch.nonzero(refs.empty)[:, 2].tolist()))
    assert empty_rows == d.empty_rows and bool(refs.empty[:, :, d.empty_rows].all())
    if c.kind == "flat" and not c.dense:
        count = spec.allowed.sum(-1).double()
        assert float((spec.lse[live] - torch.log(count).expand_as(spec.lse)[live]).abs().max()) < 1e-12
    T.attention_fwd_hold(refs.f32, refs, f"float32 of {T.attention_fwd_case_id(r)}")
    if refs.model is not None:      # (the model speaks of tile rows: the one-row kernel of the tail rows is exact fp32)
        T.attention_fwd_hold(refs.model, T.attention_fwd_refs(r, d, 0) if refs.tail else refs, f"model of {T.attention_fwd_case_id(r)}")


# (mutant of the float32 evaluation, which cases can show it)
MUTANTS = {
    "relative index off by one": (dict(rel_shift=1), lambda c: c.table and c.kind != "flat"),
    "Ck and Cq exchanged": (dict(swap_c=True), lambda c: c.table and c.Cq != c.Ck and c.kind != "flat"),
    "j < i for the causal predicate": (dict(strict_causal=True), lambda c: c.mask == 1),
    "relative term unscaled": (dict(rel_unscaled=True), lambda c: c.table and c.kind != "flat"),
    "dense mask on disallowed pairs only": (dict(dense_on_disallowed=True), lambda c: c.dense),
    "lse in base 2": (dict(lse_base2=True), lambda c: True),
    "kept logits without the mask term": (dict(logits_no_mask=True), lambda c: c.dense),
    "last key of a ragged tile dropped": (dict(drop_last_key=True), lambda c: c.Sk % 32 != 0),
    "late maximum's tile weighted by the stale maximum": (dict(stale_max=True), lambda c: c.kind == "late_max" and c.Sk > 32),
}


def _rejected(got, refs, what):
    try:
        T.attention_fwd_hold(got, refs, what)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", list(MUTANTS))
def test_hold_rejects_the_mutant(name):
    """Every mutant of the float32 evaluation is rejected on committed cases: on most of those that can show it (a table of
    one row, or a late maximum that arrives before the last tile under a mask, hides one), and never on none."""
    kw, shows = MUTANTS[name]
    tried = rejected = 0
    for c in CASES:
        if c.persistent or not shows(c):
            continue
        r, d, refs = _refs(c)
        tried += 1
        rejected += _rejected(T.attention_fwd_f32(*_args(r, d), **kw), refs, f"{name} on {T.attention_fwd_case_id(r)}")
    print(f"{name}: rejected on {rejected} of {tried} cases")
    assert rejected >= 1 and 2 * rejected >= tried


def test_hold_rejects_a_three_term_model_without_its_lo_hi_term():
    tried = rejected = 0
    for c in CASES:
        if c.persistent or c.prec != 1 or c.kind == "flat":
            continue
        r, d, refs = _refs(c)
        tried += 1
        rejected += _rejected(T.attention_fwd_model(*_args(r, d), 1, drop="lo_hi"), refs, T.attention_fwd_case_id(r))
    assert rejected >= 3 and 2 * rejected >= tried


def test_hold_rejects_wrong_empty_rows_and_finite_values_for_minus_infinity():
    c = next(c for c in CASES if c.dense and c.prec)
    r, d, refs = _refs(c)
    good = refs.f32
    T.attention_fwd_hold(good, refs, "unchanged")
    row = d.empty_rows[0]
    lse = good.lse.clone()
    lse[:, :, row] = 0.0
    with pytest.raises(AssertionError, match="1e30"):
        T.attention_fwd_hold(good._replace(lse=lse), refs, "empty row with a finite lse")
    out = good.out.clone()
    out[0, 0, row, 0] = 1e-30
    with pytest.raises(AssertionError, match="not 0"):
        T.attention_fwd_hold(good._replace(out=out), refs, "empty row with a non-zero out")
    lg = good.logits2.clone()
    lg[lg == float("-inf")] = -1e30
    with pytest.raises(AssertionError, match="-inf"):
        T.attention_fwd_hold(good._replace(logits2=lg), refs, "-1e30 for -inf")
    nan = good.out.clone()
    nan[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        T.attention_fwd_hold(good._replace(out=nan), refs, "NaN")


def _trace_cases():
    for line in pathlib.Path(EXPECTED).read_text().splitlines():
        if line.startswith("#"):
            continue
        cid, rc, n, _, kinds = line.split()
        f = cid.split("/")
        if f[F_ENTRY] == "f" and int(rc) == 0:
            yield cid, f, int(n), ({} if kinds == "-" else {k: int(v) for k, v in (kv.split(":") for kv in kinds.split(","))})


def test_route_restatement_agrees_with_the_committed_trace():
    """Case ids by the field layout of tests/test_attention_plan_host.py; family, tail launch and launch count against the
    trace's launches per launcher.  Workspace field (tests/attention_plan_tracer.cpp): 0 none; 1, 3 given; 2, 4 brought iff
    the size query answers (an accepted call with w2 or w3 is one the plane-staged route did not take)."""
    seen = set()
    for cid, f, n, kinds in _trace_cases():
        hd, prec, mask, dense, table = (int(f[i][1:] if i != F_HD else f[i][2:]) for i in (F_HD, F_PREC, F_MASK, F_DENSE, F_TABLE))
        Cq, Ck = (int(x) for x in f[F_EVENTS][1:].split("."))
        Sq, Sk = (int(x) for x in f[F_LEN][1:].split("."))
        B, H, cus, knobs, w = int(f[F_B][1:]), int(f[F_H][1:]), int(f[F_CUS][1:]), int(f[F_KNOBS][1:]), int(f[F_WS][1:])
        Ek = -(-Sk // Ck)
        ws = {0: "none", 1: "given", 3: "given", 2: "query", 4: "query"}[w]
        family, tail, nW = T.attention_fwd_route(hd, prec, Cq, Ck, table, Sq, mask, dense, ws, knobs & 3, cus, B, H, Sk=Sk,
                                                 rel_rows=-(-Sq // Cq) + Ek - 1 if table else 0)
        want = {"exact": {"attn_fwd_exact": 1}, "tiles64": {"attn_fwd2": 1}, "planes": {"attn_pack": 1, "attn_fwd3": 1}}[family]
        if tail:
            want["attn_fwd_tail_rows"] = 1
        assert kinds == want and n == sum(want.values()), cid
        assert 1 <= nW <= -(-Sq // T.ATTN_QB)
        seen.add((family, bool(tail)))
    assert seen == {("exact", False), ("tiles64", False), ("tiles64", True), ("planes", False), ("planes", True)}


def test_persistent_cases_resolve_to_the_two_schedules():
    for cus in (HOST_CUS, 104, 256, 304):
        for c in CASES:
            if c.persistent:
                r = T.attention_fwd_case_resolve(c, cus)
                blocks, (_, _, nW) = -(-c.Sq // T.ATTN_QB), T.attention_fwd_case_route(c, cus)
                assert blocks >= 3 and c.mask in (1, 2)
                assert (nW == 1 and r.B * r.H > cus) if c.persistent == "one" else (1 < nW < blocks and r.B * r.H * blocks > cus >= 2 * r.B * r.H)


def test_case_table_covers_its_requirements():
    assert T.attention_fwd_coverage_gaps(CASES) == []
    assert T.attention_fwd_coverage_gaps(CASES, HOST_CUS) == []
    assert len(set(IDS)) == len(IDS)
    unit = lambda c: c.Cq == 1 and c.Ck == 1
    one_inst = [c for c in CASES if not (T.attention_fwd_case_route(c)[0] == "tiles64" and c.hd == 32 and c.prec == 3 and not unit(c))]
    assert "inst tiles64 hd32 p3 general" in T.attention_fwd_coverage_gaps(one_inst)
    gaps = T.attention_fwd_coverage_gaps([c for c in CASES if c.mask != 2])
    assert all(f"{fam}: mask 2" in gaps for fam in T.ATTN_FAMILIES)
    assert T.attention_fwd_coverage_gaps([c for c in CASES if not c.persistent]) != []
    assert all(c.B * c.H <= 12 and c.Sq <= 400 and c.Sk <= 400 for c in CASES if not c.persistent)
    assert len(T.ATTENTION_FWD_ENTRY_CASES) >= 3
