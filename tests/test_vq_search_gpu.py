"""The stand-alone codebook searches (vq_nearest_kernel<D>, D = 8, 16, 32, 64, and vq_nearest_f16x3_kernel of
csrc/vq_nearest.hip, with the distance stage of csrc/vq_dist.h) and pack_codebook_kernel (csrc/pack.hip) against the float64
specification of tests/tests_support.py (vq_search_spec: the search half of the fused specification on a given z), at their
own entry points through ctypes: isi_pack_codebook_f32, isi_vq_nearest_f32 (the exact route), isi_vq_nearest_flags_f32
(ISI_CONV_F16X3: the split-f16 route), isi_vq_num_partials and isi_vq_finalize_f32.  The table TS.VQ_SEARCH_CASES: per route
and D codebooks of 1 code to the route's K_max (1 to 5 tiles of 32 codes, ragged last tiles, 545 codes on the split-f16
route alone), 1 to 257 vectors and one launch of 65 793 (a second grid-stride pass), a row equal to a code, the zero
vector and one of norm 1e-3, duplicate codes within a tile and across tiles, NaN / +Inf / -Inf rows and one beyond the
split-f16 range, non-finite codes, far codes of every kind (certified, scanned, in the padded tile, nothing but far codes).

The case data has no near-tie (gap >= 1e-4 of |z|^2 + |e|^2: tests_support.vq_search_settle says why that suffices for the
split-f16 ranking too), so every index must equal the spec's.  Per case: idx and the histogram exactly, the histogram ON TOP
of what counts held (k % 7); q within one float32 ulp of max(|z|, |e|) of e_idx; every partial of the squared error written
and their sum within 1e-5 of the spec's; isi_vq_finalize_f32 on the launch's partials and histogram; a lost row's
workgroup, and no other, has a NaN partial.  Every output lies in a buffer of NaN (integers: a sentinel) whose guards
must keep their bits, and every input must be unchanged.  Further: the two routes of D = 64 give the same bits of q
wherever their indices agree; a row's answer does not depend on where in the launch it stands; isi_pack_codebook_f32 is the
bit-exact transpose with |e|^2 held to the float64 sum; every refusal returns its error code before a launch and writes
nothing.  tests/test_vq_search_host.py shows, without a GPU, what the comparisons reject.

A recording aid, not a check: with ISI_VQ_SEARCH_RECORD=<file> in the environment every comparison's error, yardstick and
ratio are written there when the module ends, the worst ratio first (profiles/vq_search_checks.txt is such a run on an
MI355X: the worst ratio there is 1.27, e2 at D = 32, K = 256; diff and perplexity stay at or below 1)."""
import os

import pytest
import torch

import tests_support as TS
from test_prior_gpu import _dev

pytestmark = pytest.mark.gpu

PAD = 64                       # guard elements in front of and behind every buffer (16-byte alignment stays)
NAN = float("nan")
SENTINEL = -7777               # idx before a launch (no NaN among integers)
COUNT_GUARD = 2 ** 30
F16X3 = 8                      # ISI_CONV_F16X3
E_INVALID, E_UNSUPPORTED = -1, -4
RECORD = []                    # RowCheck of every comparison of this process
CASES = TS.VQ_SEARCH_CASES


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_VQ_SEARCH_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# kernel error, yardstick (floored at 2^-23) and their ratio against the float64 spec, per comparison of\n"
                f"# tests/test_vq_search_gpu.py; metric and bound: tests_support.compare_rows (ratio <= {TS.ROW_OPS_MARGIN:g}).  Worst ratio first.\n")
        for c in sorted(RECORD, key=lambda r: -r.ratio):
            f.write(f"{c.ratio:8.3f}  err {c.err:.3e}  yardstick {c.yardstick:.3e}  {c.what}\n")


def _lib():
    from interactive_spectrogram_inpainting import _hip
    return _hip.lib(), _dev()


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))


class Buf:
    """n elements inside a flat buffer of `fill`, PAD elements in front and behind; `src` fills the view."""

    def __init__(self, n, dev, fill=NAN, dtype=torch.float32, src=None):
        self.buf = torch.full((PAD + n + PAD,), fill, dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + n]
        if src is not None:
            self.view.copy_(src.reshape(-1))
        self.before = self.buf.clone()
        self.ptr = self.view.data_ptr()

    def intact(self):
        """The guards keep their bits."""
        return _same(self.buf[:PAD], self.before[:PAD]) and _same(self.buf[-PAD:], self.before[-PAD:])

    def untouched(self):
        return _same(self.buf, self.before)

    def cpu(self, *shape):
        return self.view.cpu().reshape(*shape) if shape else self.view.cpu()


def _check_row(what, got, ref, yard):
    err, y = TS.row_error(got, ref), max(TS.row_error(yard, ref), TS.ROW_OPS_FLOOR)
    RECORD.append(TS.RowCheck(what, err, y, err / y))                                   # (recorded whether it passes or not)
    print(f"{what}: err {err:.3e} yardstick {y:.3e} ratio {err / y:.3f}")
    TS.compare_rows(got, ref, yard, what)


class Codebook:
    """embed [D, K] on the device and what isi_pack_codebook_f32 makes of it, both outputs in guarded buffers."""

    def __init__(self, L, dev, embed):
        D, K = embed.shape
        self.D, self.K = D, K
        self.embed = Buf(D * K, dev, src=embed)
        self.codes, self.e2 = Buf(K * D, dev), Buf(K, dev)
        assert L.isi_pack_codebook_f32(self.embed.ptr, self.codes.ptr, self.e2.ptr, D, K, None) == 0, L.isi_last_error()
        torch.cuda.synchronize()
        assert self.codes.intact() and self.e2.intact() and self.embed.untouched(), "isi_pack_codebook_f32 wrote outside its outputs"
        for b in (self.codes, self.e2):
            b.before = b.buf.clone()


class Outputs:
    def __init__(self, N, D, K, dev):
        self.N, self.D, self.K = N, D, K
        self.idx = Buf(N, dev, SENTINEL, torch.int64)
        self.q = Buf(N * D, dev)
        self.start = (torch.arange(K) % 7).to(torch.int32)                  # counts is accumulated into, not written
        self.counts = Buf(K, dev, COUNT_GUARD, torch.int32, self.start)
        self.part = Buf(TS.vq_num_partials(N), dev)

    def all(self):
        return {"idx": self.idx, "q": self.q, "counts": self.counts, "sse_part": self.part}

    def assert_guards(self, what):
        for name, b in self.all().items():
            assert b.intact(), f"{what}: the kernel wrote outside {name}"

    def assert_untouched(self, what):
        for name, b in self.all().items():
            assert b.untouched(), f"{what}: a refused launch wrote to {name}"

    def histogram(self):
        return self.counts.cpu().long() - self.start.long()


def _call(L, route, z, codes, e2, idx, q, counts, part, N, D, K):
    if route == TS.VQ_F16X3:
        rc = L.isi_vq_nearest_flags_f32(z, codes, e2, idx, q, counts, part, N, D, K, F16X3, None)
    else:
        rc = L.isi_vq_nearest_f32(z, codes, e2, idx, q, counts, part, N, D, K, None)
    torch.cuda.synchronize()
    return rc


def _search(L, dev, route, z, book, what):
    """One launch of `route` on z [N, D] (CPU) and a Codebook; returns its Outputs, guards and inputs checked."""
    N, D = z.shape
    assert D == book.D
    zb = Buf(N * D, dev, src=z)
    out = Outputs(N, D, book.K, dev)
    rc = _call(L, route, zb.ptr, book.codes.ptr, book.e2.ptr, out.idx.ptr, out.q.ptr, out.counts.ptr, out.part.ptr, N, D, book.K)
    assert rc == 0, f"{what}: {L.isi_last_error()}"
    out.assert_guards(what)
    assert zb.untouched() and book.codes.untouched() and book.e2.untouched(), f"{what}: the launch changed one of its inputs"
    return out


def _hold(L, dev, out, refs, what):
    """Every assertion on one launch's outputs against a VqSearchRefs-like `refs` (its .spec)."""
    spec, (N, D, K) = refs.spec, (out.N, out.D, out.K)
    n_part = L.isi_vq_num_partials(N)
    assert n_part == TS.vq_num_partials(N) == out.part.view.numel()
    TS.vq_fused_hold_idx(out.idx.cpu(), spec, what)
    TS.vq_fused_hold_counts(out.histogram(), spec, what)
    TS.vq_fused_hold_q(out.q.cpu(N, D), refs, what)
    part = out.part.cpu()
    TS.vq_fused_hold_sse(part, spec, what)
    live = spec.idx >= 0
    want = TS.vq_fused_partials(spec.sse_rows)
    assert torch.equal(torch.isnan(part), torch.isnan(want)), f"{what}: a lost row's workgroup, and no other, has a NaN partial"
    ok = ~torch.isnan(want)
    assert bool(torch.isfinite(part[ok]).all()) and bool((part[ok] >= 0).all())
    if not bool(live.all()):
        assert int(out.histogram().sum()) == int(live.sum()), f"{what}: a lost row was counted"
        total, ref = float(part[ok].double().sum()), float(want[ok].sum())
        assert abs(total - ref) <= TS.VQ_FUSED_SSE_RTOL * ref, f"{what}: the workgroups without a lost row sum to {total!r} against {ref!r}"
        return
    # isi_vq_finalize_f32 on the launch's own partials and histogram
    hist = Buf(K, dev, COUNT_GUARD, torch.int32, out.histogram().to(torch.int32))
    out2 = Buf(2, dev)
    assert L.isi_vq_finalize_f32(out.part.ptr, n_part, hist.ptr, K, N, D, out2.ptr, None) == 0, L.isi_last_error()
    torch.cuda.synchronize()
    assert out2.intact() and hist.untouched() and out.part.intact()
    counts = hist.cpu()
    ref, yard = TS.vq_finalize_spec(part, counts, N, D), TS.vq_finalize_f32(part, counts, N, D)
    _check_row(f"{what} diff", out2.cpu()[0:1], ref[0], yard[0])
    _check_row(f"{what} perplexity", out2.cpu()[1:2], ref[1], yard[1])
    assert abs(float(out2.cpu()[0]) - float(spec.diff)) <= 2 * TS.VQ_FUSED_SSE_RTOL * float(spec.diff)


# --------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("case", CASES, ids=TS.vq_search_case_id)
def test_search_holds_the_spec(case):
    L, dev = _lib()
    refs, name = TS.vq_search_case_refs(case), TS.vq_search_case_id(case)
    if case.N > 65536:         # the second grid-stride pass: more tiles than workgroups, the last one ragged
        assert L.isi_vq_num_partials(case.N) == TS.VQ_FUSED_GRID and -(-case.N // TS.VQ_FUSED_TILE) > TS.VQ_FUSED_GRID and case.N % TS.VQ_FUSED_TILE
    book = Codebook(L, dev, refs.embed)
    out = _search(L, dev, case.route, refs.z, book, name)
    _hold(L, dev, out, refs, name)
    idx = out.idx.cpu()
    if case.kind == "dups":
        sources, copies = TS.vq_search_dup_layout(case.K)
        for src, cs, row in zip(sources, copies, TS.VQ_SEARCH_DUP_ROWS):
            assert int(idx[row]) == src and not bool(torch.isin(idx, torch.tensor(cs)).any()), f"{name}: the lowest index wins"
    for row, code in TS.VQ_SEARCH_FAR_ROWS.get(case.kind, {}).items():
        assert int(idx[row]) == code
    if case.kind == "lost" and case.route == TS.VQ_EXACT:
        assert int(idx[TS.VQ_SEARCH_LOUD_ROW]) == TS.VQ_SEARCH_LOUD_CODE, "the exact route has no operand range beyond fp32's own"


# ------------------------------------------------------------------------------------------------- between the two routes
@pytest.mark.parametrize("K,N,kind", [(100, 257, "plain"), (96, 257, "plain"), (160, 257, "plain"), (100, 257, "edges"),
                                      (512, 257, "dups"), (100, 600, "lost")])
def test_routes_of_d64_agree(K, N, kind):
    L, dev = _lib()
    ce, cs = TS.VqSearchCase(TS.VQ_EXACT, 64, K, N, kind), TS.VqSearchCase(TS.VQ_F16X3, 64, K, N, kind)
    assert ce in CASES and cs in CASES
    re_, rs = TS.vq_search_case_refs(ce), TS.vq_search_case_refs(cs)
    assert _same(re_.z, rs.z) and _same(re_.embed, rs.embed)
    book = Codebook(L, dev, re_.embed)
    oe, os_ = _search(L, dev, TS.VQ_EXACT, re_.z, book, "exact"), _search(L, dev, TS.VQ_F16X3, rs.z, book, "f16x3")
    ie, is_ = oe.idx.cpu(), os_.idx.cpu()
    differ = (ie != is_).nonzero().reshape(-1).tolist()
    assert differ == ([TS.VQ_SEARCH_LOUD_ROW] if kind == "lost" else []), "the routes agree except on the row beyond the split-f16 range"
    agree = ie == is_
    assert _same(oe.q.cpu(N, 64)[agree], os_.q.cpu(N, 64)[agree]), "q of the two routes differs in bits where their indices agree"
    if kind != "lost":
        assert _same(oe.counts.view, os_.counts.view)


# ------------------------------------------------------------------------------------------------ position independence
@pytest.mark.parametrize("case", [TS.VqSearchCase(TS.VQ_EXACT, 32, 100, 257, "edges"), TS.VqSearchCase(TS.VQ_F16X3, 64, 100, 257, "edges")],
                         ids=TS.vq_search_case_id)
def test_answer_does_not_depend_on_the_position(case):
    L, dev = _lib()
    assert case in CASES
    refs = TS.vq_search_case_refs(case)
    perm = torch.randperm(case.N, generator=torch.Generator().manual_seed(case.D))
    assert int((perm // 32 != torch.arange(case.N) // 32).sum()) > case.N // 2, "most rows change their wave"
    book = Codebook(L, dev, refs.embed)
    a = _search(L, dev, case.route, refs.z, book, "in order")
    b = _search(L, dev, case.route, refs.z[perm].contiguous(), book, "permuted")
    assert torch.equal(b.idx.cpu(), a.idx.cpu()[perm]), "a row's index moved with its position"
    assert _same(b.q.cpu(case.N, case.D), a.q.cpu(case.N, case.D)[perm]), "a row's q changed bits with its position"
    assert torch.equal(a.histogram(), b.histogram())


# ------------------------------------------------------------------------------------------------------- pack_codebook
@pytest.mark.parametrize("D", TS.VQ_SEARCH_DIMS)
@pytest.mark.parametrize("K", [1, 255, 256, 257, "K_max"])
def test_pack_codebook(D, K):
    L, dev = _lib()
    K = TS.vq_search_k_max(D) if K == "K_max" else K
    embed = torch.randn(D, K, generator=torch.Generator().manual_seed(D * 10007 + K))
    book = Codebook(L, dev, embed)                         # (guards and the input: checked there)
    codes, e2 = TS.vq_pack_codebook_spec(embed)
    assert _same(book.codes.cpu(K, D), codes), "codes is not the bit-exact transpose"
    _check_row(f"pack_codebook D={D} K={K} e2", book.e2.cpu(K, 1), e2, TS.vq_pack_codebook_f32(embed))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_k_max_is_accepted_and_one_more_refused():
    L, dev = _lib()
    for route, D in TS.VQ_SEARCH_ROUTES:
        split = route == TS.VQ_F16X3
        k_max = TS.vq_search_k_max(D, split)
        k_over = 577 if split else k_max + 1               # (577 with the flag falls to the exact kernel, which refuses it too)
        assert k_over == k_max + 1
        embed = torch.randn(D, k_over, generator=torch.Generator().manual_seed(D))
        book = Codebook(L, dev, embed)
        z = Buf(33 * D, dev, src=torch.randn(33, D, generator=torch.Generator().manual_seed(1)))
        out = Outputs(33, D, k_over, dev)
        rc = _call(L, route, z.ptr, book.codes.ptr, book.e2.ptr, out.idx.ptr, out.q.ptr, out.counts.ptr, out.part.ptr, 33, D, k_over)
        assert rc == E_UNSUPPORTED, f"{route} D={D} K={k_over}: returned {rc}"
        out.assert_untouched(f"{route} D={D} K={k_over}")
        assert z.untouched() and book.codes.untouched() and book.e2.untouched()
        # (K_max itself: test_search_holds_the_spec runs it on every route; here the same buffers, one code fewer)
        rc = _call(L, route, z.ptr, book.codes.ptr, book.e2.ptr, out.idx.ptr, out.q.ptr, out.counts.ptr, out.part.ptr, 33, D, k_max)
        assert rc == 0, f"{route} D={D} K={k_max}: {L.isi_last_error()}"
        out.assert_guards(f"{route} D={D} K={k_max}")
        assert bool((out.idx.cpu() >= 0).all()) and bool((out.idx.cpu() < k_max).all())


def test_refusals_write_nothing():
    L, dev = _lib()
    N, D, K = 33, 64, 40
    g = torch.Generator().manual_seed(2)
    # buffers large enough for every shape asked for below (D = 128), so that no refused call names memory it does not own
    book = Codebook(L, dev, torch.randn(128, K, generator=g))
    z = Buf(N * 128, dev, src=torch.randn(N * 128, generator=g))
    out = Outputs(N, 128, K, dev)
    args = dict(z=z.ptr, codes=book.codes.ptr, e2=book.e2.ptr, idx=out.idx.ptr, q=out.q.ptr, counts=out.counts.ptr, part=out.part.ptr,
                N=N, D=D, K=K)
    refused = {"D = 24": (dict(D=24), E_UNSUPPORTED), "D = 128": (dict(D=128), E_UNSUPPORTED),
               "N = 0": (dict(N=0), E_INVALID), "K = 0": (dict(K=0), E_INVALID),
               "z offset by one float": (dict(z=z.ptr + 4), E_INVALID),
               "codes_kd offset by one float": (dict(codes=book.codes.ptr + 4), E_INVALID),
               "q_out offset by one float": (dict(q=out.q.ptr + 4), E_INVALID)}
    for p in ("z", "codes", "e2", "idx", "q", "counts", "part"):
        refused[f"{p} is NULL"] = ({p: None}, E_INVALID)
    for route in (TS.VQ_EXACT, TS.VQ_F16X3):
        for what, (over, code) in refused.items():
            a = dict(args)
            a.update(over)
            rc = _call(L, route, a["z"], a["codes"], a["e2"], a["idx"], a["q"], a["counts"], a["part"], a["N"], a["D"], a["K"])
            assert rc == code, f"{route}, {what}: returned {rc}, expected {code}"
            out.assert_untouched(f"{route}, {what}")
            assert z.untouched() and book.codes.untouched() and book.e2.untouched(), what
    # the same arguments are accepted as they stand
    for route in (TS.VQ_EXACT, TS.VQ_F16X3):
        assert _call(L, route, *(args[k] for k in ("z", "codes", "e2", "idx", "q", "counts", "part", "N", "D", "K"))) == 0, L.isi_last_error()
        out.assert_guards(route)
