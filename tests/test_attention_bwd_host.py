"""The float64 specification of the relative-attention backward (tests/tests_support.py), held on the host: against float64
autograd of the float64 forward and oracle/prior_oracle.py, against its own yardsticks, and against mutants -- what the hold
of tests/test_attention_bwd_gpu.py rejects.  The route restatement is held to the committed launch trace
(tests/attention_plan_trace.txt), the case table to its requirements.  No GPU, no compiler."""
import functools
import math
import pathlib

import pytest
import torch

import tests_support as T
from test_attention_plan_host import (EXPECTED, F_B, F_DENSE, F_ENTRY, F_EVENTS, F_GEMM, F_H, F_HD, F_KNOBS, F_LEN, F_LOGITS, F_MASK,
                                      F_PREC, F_STRIDES, F_TABLE)

HOST_CUS = 8          # persistent cases are resolved for a small device here: the same grids at a fraction of the pairs
CASES = T.ATTENTION_BWD_CASES
IDS = [T.attention_bwd_case_id(c) for c in CASES]


@functools.lru_cache(maxsize=None)
def _refs(c):
    """(resolved case, data, refs): the outputs are small, every case's are kept for the mutants"""
    r = T.attention_bwd_case_resolve(c, HOST_CUS)
    d = T.attention_bwd_case_data(r)
    return r, d, T.attention_bwd_refs(r, d, T.attention_bwd_case_route(c, HOST_CUS))


def _autograd(c, d):
    """dq, dk, dv, d_rel by float64 autograd through a float64 softmax attention on the case's float32 inputs (the masked
    softmax written out, so that an empty row is 0 and differentiable)."""
    q, k, v, dout = (t.double().permute(1, 2, 0, 3).clone().requires_grad_(True) for t in (d.q, d.k, d.v, d.dout))
    rel = None if d.rel is None else d.rel.double().clone().requires_grad_(True)
    logits = q @ k.transpose(-1, -2)
    if rel is not None:
        idx = T.attention_rel_index(c.Sq, c.Sk, c.Cq, c.Ck, d.Ek).expand(c.B, c.H, c.Sq, c.Sk)
        logits = logits + torch.einsum("bhid,hrd->bhir", q, rel).gather(3, idx)
    logits = logits * d.scale
    if d.dense is not None:
        logits = logits + d.dense.double()
    live = T.attention_allowed(c.Sq, c.Sk, c.mask) & (logits.detach() > float("-inf"))
    safe = torch.where(live, logits, torch.zeros_like(logits))
    m = torch.where(live, logits.detach(), torch.full_like(logits, float("-inf"))).amax(-1, keepdim=True)
    p = torch.where(live, torch.exp(safe - torch.where(torch.isfinite(m), m, torch.zeros_like(m))), torch.zeros_like(logits))
    s = p.sum(-1, keepdim=True)
    out = (p / torch.where(s > 0, s, torch.ones_like(s))) @ v
    (out * dout.detach()).sum().backward()
    return T.AttnBwd(q.grad, k.grad, v.grad, None if rel is None else rel.grad)


AUTOGRAD_CASES = [c for c in CASES if not c.persistent]


@pytest.mark.parametrize("c", AUTOGRAD_CASES, ids=[T.attention_bwd_case_id(c) for c in AUTOGRAD_CASES])
def test_spec_equals_float64_autograd_up_to_the_rounding_of_the_given_tensors(c):
    """The spec is a function of the GIVEN out, lse (and kept logits); handed the float32 roundings of the float64 forward's,
    it differs from autograd through that forward by that rounding alone.  The distance, in the row metric of the hold, stays
    under the float32 yardstick's own error on the same data; handed the unrounded float64 tensors it is autograd's result."""
    d = T.attention_bwd_case_data(c, forced=False)
    route = T.attention_bwd_case_route(c, HOST_CUS)
    want = _autograd(c, d)
    fwd = T.attention_fwd_spec(d.q, d.k, d.v, d.rel, c.H, c.Cq, c.Ck, d.Ek, c.mask, d.dense, d.scale)
    # (kept logits are handed over unrounded here: the distance measured is that of the rounded out and lse)
    a = T.attention_bwd_args(c, d, False)[:14] + (fwd.logits2 if route.saved else None,)
    spec, f32 = T.attention_bwd_spec(*a), T.attention_bwd_f32(*a)
    exact = T.attention_bwd_spec(*a[:12], fwd.out.permute(2, 0, 1, 3), fwd.lse, a[14])
    for name in T.AttnBwd._fields:
        w = getattr(want, name)
        if w is None:
            assert getattr(spec, name) is None
            continue
        # a row whose gradient vanishes identically (dO v = D where a query has a single live key: one key, the first causal
        # row) is rounding noise against 0 on every side: held absolutely, and left out of the row metric it would swamp
        rows = w.abs().amax(-1) > 1e-9
        for t in (exact, spec):
            assert float(getattr(t, name)[~rows].abs().max() if not bool(rows.all()) else 0.0) < 1e-9, name
        if not bool(rows.any()):
            continue
        w = w[rows]
        dist, yard = T.row_error(getattr(spec, name)[rows], w), max(T.row_error(getattr(f32, name)[rows], w), T.ROW_OPS_FLOOR)
        # (float64 rounds 2^-29 as coarsely as float32: on the unrounded tensors the two float64 evaluations differ by their
        # own rounding alone, whatever the conditioning of a saturated row prices into both)
        assert T.row_error(getattr(exact, name)[rows], w) < 1e-6 * yard, name
        print(f"{name}: spec of the rounded tensors against autograd {dist:.3e}, float32 evaluation {yard:.3e}")
        assert dist <= yard, f"{name}: {dist:.3e} against {yard:.3e}"


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("table", [True, False])
def test_spec_equals_autograd_through_the_oracle_on_self_attention(mode, table):
    """oracle/prior_oracle.py::attention with identity projections: x.grad = dq + dk + dv, rel_embeddings.grad = d_rel."""
    from oracle import prior_oracle as P
    from test_attention_fwd_host import _mask
    torch.manual_seed(11 + mode)
    S, B, H, hd, C = 40, 2, 3, 16, 4
    dm, E = H * hd, S // C
    x = torch.randn(S, B, dm, dtype=torch.float64, requires_grad=True)
    rel = torch.randn(H, 2 * E - 1, hd, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(S, B, dm, dtype=torch.float64)
    eye = torch.eye(dm, dtype=torch.float64)
    sd = {"in_proj_weight": torch.cat([eye, eye, eye]), "in_proj_bias": torch.zeros(3 * dm, dtype=torch.float64), "out_proj.weight": eye,
          "out_proj.bias": torch.zeros(dm, dtype=torch.float64), "rel_embeddings": rel}
    out = P.attention(x, x, sd, "", H, C, E, C, E, _mask(mode, S, S), bias=table)
    (out * dout).sum().backward()
    xd = x.detach()
    scale = 1.0 / math.sqrt(hd)
    fwd = T.attention_fwd_spec(xd, xd, xd, rel.detach() if table else None, H, C, C, E, mode, None, scale)
    got = T.attention_bwd_spec(xd, xd, xd, rel.detach() if table else None, H, C, C, E, mode, None, scale, dout, fwd.out.permute(2, 0, 1, 3), fwd.lse)
    total = (got.dq + got.dk + got.dv).permute(2, 0, 1, 3).reshape(S, B, dm)
    assert float((total - x.grad).abs().max()) < 1e-11
    if table:
        assert float((got.d_rel - rel.grad).abs().max()) < 1e-11


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_yardsticks_pass_the_hold_by_construction(c):
    """The float32 evaluation passes compare_rows against the spec with a ratio of at most 1, the model likewise where the
    yardstick takes it; the rows the case designs to be empty come back exactly 0; the model's distance is printed."""
    r, d, refs = _refs(c)
    what = T.attention_bwd_case_id(r)
    checks = T.attention_bwd_hold(refs.f32, refs, f"float32 of {what}")
    assert all(k.ratio <= 1.0 for k in checks.values())
    assert bool((refs.spec.dq[:, :, d.empty_rows] == 0).all())
    if d.rel is not None:
        idx, allowed = T.attention_rel_index(r.Sq, r.Sk, r.Cq, r.Ck, d.Ek), T.attention_allowed(r.Sq, r.Sk, r.mask)
        never = torch.ones(d.rel_rows, dtype=torch.bool)
        never[idx[allowed]] = False
        assert bool((refs.spec.d_rel[:, never] == 0).all())
        lo, n = refs.route.rho
        assert bool(never[:lo].all()) and bool(never[lo + n:].all())
        if r.ek_extra and r.mask == 0:
            assert int(never.sum()) >= r.ek_extra
    if refs.model is not None:
        for name in T.AttnBwd._fields:
            if getattr(refs.spec, name) is not None:
                print(f"model p{r.prec}{' kept logits' if r.saved else ''} {name}: {T.row_error(getattr(refs.model, name), getattr(refs.spec, name)):.3e} "
                      f"(float32 evaluation {T.row_error(getattr(refs.f32, name), getattr(refs.spec, name)):.3e})")
        if not (refs.route.tail_q or refs.route.tail_k):
            assert all(k.ratio <= 1.0 for k in T.attention_bwd_hold(refs.model, refs, f"model of {what}").values())


def _route(c):
    return T.attention_bwd_case_route(c, HOST_CUS)


# mutant of the float32 evaluation -> (keywords given the case's route, which cases can show it)
MUTANTS = {
    "D left out of dS": (lambda r: dict(no_D=True), lambda c: True),
    "scale missing from dS": (lambda r: dict(no_scale=True), lambda c: True),
    "scale applied a second time to the G E share of dQ": (lambda r: dict(scale_twice_ge=True), lambda c: c.table and c.kind != "flat"),
    "r(i,j) off by one": (lambda r: dict(rel_shift=1), lambda c: c.table and c.Sq > 1),
    "Cq and Ck exchanged in G": (lambda r: dict(swap_c_in_g=True), lambda c: c.table and c.Cq != c.Ck),
    "the causal diagonal excluded": (lambda r: dict(strict_causal=True), lambda c: c.mask == 1),
    "last key of a ragged 32-key tile left out of dK / dV": (lambda r: dict(drop_last_key=True), lambda c: c.Sk % 32 != 0),
    "a tail query writes dQ but not its row of G": (lambda r: dict(g_drop_last_query=True), lambda c: c.table and _route(c).tail_q > 0),
    "query 128 left out of dE": (lambda r: dict(de_drop_query=128), lambda c: c.table and c.Sq > 128),
    "last batch item left out of dE": (lambda r: dict(de_drop_last_batch=True), lambda c: c.table),
    "d_rel rows outside rho not zeroed": (lambda r: dict(junk_outside_rho=r.rho),
                                          lambda c: c.table and _route(c).rho[1] < -(-c.Sq // c.Cq) + -(-c.Sk // c.Ck) + c.ek_extra - 1),
}
PER_MUTANT = 8        # cases tried per mutant: the first that can show it


def _rejected(got, refs, what):
    try:
        T.attention_bwd_hold(got, refs, what)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", list(MUTANTS))
def test_hold_rejects_the_mutant(name):
    """Every mutant of the float32 evaluation is rejected on committed cases: a case that can show it exists, and most of
    those tried reject it."""
    kw, shows = MUTANTS[name]
    picked = [c for c in CASES if not c.persistent and shows(c)][:PER_MUTANT]
    assert picked, "no case of the table can show this mutant"
    rejected = 0
    for c in picked:
        r, d, refs = _refs(c)
        got = T.attention_bwd_f32(*T.attention_bwd_args(r, d, refs.route.saved), **kw(refs.route))
        rejected += _rejected(got, refs, f"{name} on {T.attention_bwd_case_id(r)}")
    print(f"{name}: rejected on {rejected} of {len(picked)} cases")
    assert rejected >= 1 and 2 * rejected >= len(picked)


def test_hold_rejects_a_model_that_renormalises_instead_of_reading_the_given_lse():
    """The kernels must take lse as given: the row the case data empties through lse = ATTN_EMPTY_LSE alone contributes 0;
    a model that forms its own log-sum-exp of the recomputed logits gives that row a gradient."""
    picked = [c for c in CASES if not c.persistent and c.prec and c.Sq >= 33][:PER_MUTANT]
    rejected = 0
    for c in picked:
        r, d, refs = _refs(c)
        assert d.forced_row is not None and bool((refs.spec.dq[:, :, d.forced_row] == 0).all())
        ro = refs.route
        got = T.attention_bwd_model(*T.attention_bwd_args(r, d, ro.saved), r.prec, ro.saved, tail_q=ro.tail_q, tail_k=ro.tail_k,
                                    g_from_kv=ro.g_from_kv, renorm_lse=True)
        rejected += _rejected(got, refs, T.attention_bwd_case_id(r))
    print(f"renormalised lse: rejected on {rejected} of {len(picked)} cases")
    assert picked and rejected >= 1 and 2 * rejected >= len(picked)


@pytest.mark.parametrize("product", ["qk", "band", "dp", "dv", "dk", "dq", "ge", "de"])
def test_hold_rejects_a_three_term_model_without_a_lo_hi_term(product):
    shows = {"qk": lambda c: not c.saved, "band": lambda c: not c.saved and c.table, "ge": lambda c: c.table, "de": lambda c: c.table}
    picked = [c for c in CASES if not c.persistent and c.prec in (1, 3) and c.kind not in ("flat", "peaked") and c.Sq >= 33
              and shows.get(product, lambda c: True)(c)][:PER_MUTANT]
    rejected = 0
    for c in picked:
        r, d, refs = _refs(c)
        ro = refs.route
        got = T.attention_bwd_model(*T.attention_bwd_args(r, d, ro.saved), r.prec, ro.saved, tail_q=ro.tail_q, tail_k=ro.tail_k,
                                    g_from_kv=ro.g_from_kv, drop=product)
        rejected += _rejected(got, refs, f"{product} on {T.attention_bwd_case_id(r)}")
    print(f"lo.hi dropped from {product}: rejected on {rejected} of {len(picked)} cases")
    assert picked and rejected >= 1


def test_hold_rejects_nan_and_a_non_zero_empty_row():
    c = next(c for c in CASES if c.dense and c.prec and c.table)
    r, d, refs = _refs(c)
    good = refs.f32
    T.attention_bwd_hold(good, refs, "unchanged")
    dq = good.dq.clone()
    dq[0, 0, d.empty_rows[0], 0] = 1e-30
    with pytest.raises(AssertionError, match="not 0"):
        T.attention_bwd_hold(good._replace(dq=dq), refs, "empty row with a non-zero dq")
    dk = good.dk.clone()
    dk[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        T.attention_bwd_hold(good._replace(dk=dk), refs, "NaN")
    with pytest.raises(AssertionError):
        T.attention_bwd_hold(good._replace(d_rel=None), refs, "no d_rel")


def _trace_cases():
    for line in pathlib.Path(EXPECTED).read_text().splitlines():
        if line.startswith("#"):
            continue
        cid, rc, n, _, kinds = line.split()
        f = cid.split("/")
        if f[F_ENTRY] == "b" and int(rc) == 0:
            yield cid, f, int(n), ({} if kinds == "-" else {k: int(v) for k, v in (kv.split(":") for kv in kinds.split(","))})


def test_route_restatement_predicts_every_accepted_backward_line_of_the_committed_trace():
    """Case ids by the key at the top of tests/attention_plan_tracer.cpp; the line's `g` field is the answer its stub gave to
    gemm_split_applicable and is handed to the mirror as the override."""
    seen = set()
    for cid, f, n, kinds in _trace_cases():
        hd, prec, mask, dense, table = (int(f[i][1:] if i != F_HD else f[i][2:]) for i in (F_HD, F_PREC, F_MASK, F_DENSE, F_TABLE))
        Cq, Ck = (int(x) for x in f[F_EVENTS][1:].split("."))
        Sq, Sk = (int(x) for x in f[F_LEN][1:].split("."))
        B, H, knobs, strided, lg, g = (int(f[i][1:]) for i in (F_B, F_H, F_KNOBS, F_STRIDES, F_LOGITS, F_GEMM))
        Ek = -(-Sk // Ck)
        r = T.attention_bwd_route(hd, prec, Cq, Ck, table, Sq, Sk, B, H, mask, dense, lg == 1, strided == 0, knobs & 28, Ek,
                                  -(-Sq // Cq) + Ek - 1, gemm_ok=bool(g))
        want = T.attention_bwd_launches(r)
        assert kinds == want and n == sum(want.values()), cid
        seen.add((r.split, r.saved, r.gemm_path, r.band_only, r.g_from_kv, bool(r.tail_q or r.tail_k)))
    assert len(seen) >= 12
    for i, name in enumerate(("split", "saved", "gemm_path", "band_only", "g_from_kv", "tails")):
        assert {s[i] for s in seen} == {False, True}, name


def test_gemm_split_applicable_restated():
    """csrc/gemm_split_f32.hip: split modes 1 and 3, K a multiple of 32 and >= 128, N > 32, M >= 256 -- both sides of each."""
    table = [((256, 64, 128), True), ((255, 64, 128), False), ((256, 33, 128), True), ((256, 32, 128), False), ((256, 64, 96), False),
             ((256, 64, 160), True), ((256, 64, 144), False), ((258, 64, 288), True), ((258, 16, 288), False), ((254, 64, 256), False)]
    for (M, N, K), want in table:
        assert T.gemm_split_applicable(M, N, K, 1) is want, (M, N, K)
    assert T.gemm_split_applicable(256, 64, 128, 3) and not T.gemm_split_applicable(256, 64, 128, 0) and not T.gemm_split_applicable(256, 64, 128, 2)
    # what the issue derives from it: the GEMM back end exists for head_dim 64, Sq B >= 256 and Rp >= 128 only
    for hd, Sq, B, want in ((64, 129, 2, True), (32, 129, 2, False), (16, 385, 2, False), (64, 127, 2, False)):
        r = T.attention_bwd_route(hd, 1, 1, 1, True, Sq, Sq, B, 2, 0, False, False, True, 0, Sq, 2 * Sq - 1)
        assert r.gemm_path is want and r.band_only is want
    assert not T.attention_bwd_route(64, 1, 1, 1, True, 129, 129, 2, 2, 0, False, False, False, 0, 129, 257).gemm_path       # q_ss != B q_sb
    assert not T.attention_bwd_route(64, 0, 1, 1, True, 129, 129, 2, 2, 0, False, False, True, 0, 129, 257).gemm_path        # exact pair
    r = T.attention_bwd_route(64, 1, 1, 1, True, 129, 129, 2, 2, 1, False, True, True, 0, 129, 257)
    assert r.rho == (128, 129) and r.Rp == 160 and r.band == (0, 0, 1, 0) and r.g_from_kv
    assert (r.g_off, r.g_len) == (576, 2 * 2 * 129 * 160)


def test_case_table_covers_its_requirements():
    assert T.attention_bwd_coverage_gaps(CASES) == []
    assert T.attention_bwd_coverage_gaps(CASES, HOST_CUS) == []
    assert T.attention_bwd_coverage_gaps(CASES, 304) == []
    assert len(set(IDS)) == len(IDS)
    gaps = T.attention_bwd_coverage_gaps([c for c in CASES if c.mask != 2])
    assert all(f"{fam}: mask 2" in gaps for fam in T.ATTN_BWD_FAMILIES) and "gemm mask 2: g_from_kv" in gaps
    assert "tail query declined by Ck = 2" in T.attention_bwd_coverage_gaps([c for c in CASES if c.Ck != 2])
    assert T.attention_bwd_coverage_gaps([c for c in CASES if not c.persistent]) != []
    assert all(2 <= c.B <= 4 and 2 <= c.H <= 3 and c.Sq <= 400 and c.Sk <= 400 for c in CASES if not c.persistent)
    kinds = {(c.layout, c.Sq == c.Sk) for c in T.ATTENTION_BWD_ENTRY_CASES}
    assert ("contig", False) in kinds or ("contig", True) in kinds
    assert ("fused", True) in kinds
