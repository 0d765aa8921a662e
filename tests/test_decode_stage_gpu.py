"""The stage kernels of the key/value-cached decoding loop (csrc/prior_decode.hip: row_gemv1_kernel, row_gemvm_kernel,
row_mfma32_kernel + row_mfma_finish_kernel, row_linear_ln_kernel, single_source_cross_kernel) against the float64
specifications of tests/tests_support.py, launched as the loop launches them: through isi_decode_stage_ex_f32, which builds
the launch with the host plan's own Stage / placed() / launch_stage_rows(), and isi_decode_single_source_f32.  One case per
route of the plan and of the launchers' instantiations (DECODE_STAGE_CASES, the `stagex/` cases of the host tracer).

Every buffer sits between NaN pads (integers and bf16: a sentinel pattern), outputs start as NaN / the sentinel, and the input
rows, residual rows and cache slots at positions the case does not address hold NaN / the sentinel: a finite result with the
right values proves that the right rows were read, an unchanged sentinel that nothing else was written.  Comparisons are
`compare_rows` (ROW_OPS_MARGIN times the error of a float32 torch evaluation, per row, every element); a bf16 k|v value is
allowed half a bf16 ulp of the spec value on top (compare_rows_bf16).

The merged-input route (attention partials merged in the prologue of row_gemv1_kernel) uses __expf where the yardstick uses
the exact exponential; it stays inside ROW_OPS_MARGIN of that yardstick as it is (the module's RECORD line gives the worst
ratio per family), so the yardstick carries no extra term.

What the cases found (fixed in the host plan, csrc/prior_sample_run.cpp: row_mfma_supported): the tile kernel reduces 8 floats of
a residual row per lane, and a normalised residual of 516 features whose statistics were not handed came out 7.8e-3 of the row
maximum wrong (25 000 times the yardstick); likewise its input statistics cover K <= 2048.  Such stages now leave the tiles.

With ISI_DECODE_STAGE_RECORD=<file> the worst ratio per family is also written there (profiles/decode_stage_checks.txt)."""
import collections
import ctypes as C
import functools
import math
import os

import pytest
import torch

import tests_support as T
from test_prior_gpu import _dev

pytestmark = pytest.mark.gpu

EPS = 1e-5
PAD = 64
SENTINEL16 = 0x7FA5             # a bf16 NaN no rounding produces
POISON32 = -(2 ** 30)
RECORD = collections.defaultdict(list)      # family -> [RowCheck]
P, AT = T.DECODE_STAGE_POSITIONS, T.DECODE_STAGE_P


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    lines = []
    for family, checks in sorted(RECORD.items()):
        w = max(checks, key=lambda r: r.ratio)
        lines.append(f"RECORD decode_stage {family}: worst error / float32 yardstick {w.ratio:.3f} over {len(checks)} comparisons "
                     f"(err {w.err:.3e}, yardstick {w.yardstick:.3e}, {w.what})")
    print("\n" + "\n".join(lines))
    path = os.environ.get("ISI_DECODE_STAGE_RECORD")
    if path and lines:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _hold(family, got, ref, yard, what, bf16=False):
    r = (T.compare_rows_bf16 if bf16 else T.compare_rows)(got, ref, yard, what)
    RECORD[family].append(r)
    return r


class Buf:
    """A device array between pads of PAD elements; `fill`: what the pads and the array start as."""

    def __init__(self, shape, dev, dtype=torch.float32, fill=float("nan"), data=None):
        n = math.prod(shape)
        self.fill, self.shape = fill, tuple(shape)
        self.full = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
        self.t = self.full[PAD:PAD + n].view(self.shape)
        if data is not None:
            self.t.copy_(data.to(dtype))
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 0

    def is_fill(self, t):
        return bool(torch.isnan(t).all()) if isinstance(self.fill, float) else bool((t == self.fill).all())

    def pads_intact(self):
        return self.is_fill(self.full[:PAD]) and self.is_fill(self.full[-PAD:])


def _settle(rc, what):
    """Wait for the launch.  A launch failure or a device error is no comparison that failed: the session ends there, so that
    nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: the device reported {e}", returncode=3)
    if rc == -2:                 # ISI_E_LAUNCH
        from interactive_spectrogram_inpainting import _hip
        pytest.exit(f"{what}: launch failure: {_hip.lib().isi_last_error()}", returncode=3)


def _only_rows(full, at):
    """[P][M][W] holding `full`'s row m at position at[m] and NaN everywhere else."""
    out = torch.full_like(full, float("nan"))
    m = torch.arange(full.shape[1])
    out[at, m] = full[at, m]
    return out


Run = collections.namedtuple("Run", "rc kernel out out2 out2_raw stat bufs at")


def _launch(c, d, dev, addr=None, row_pos=None, res_stat=None):
    """One isi_decode_stage_ex_f32 call of case c on data d; everything checked that must hold whatever the values:
    pads, cache slots not addressed, the workspace of a refused side-by-side run."""
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    addr = c.addr if addr is None else addr
    rag = addr in (T.AT_ROWS, T.AT_ROWS_COUNTER)
    if rag and row_pos is None:
        row_pos = T.decode_stage_row_positions(c.M)
    at = [int(v) for v in row_pos[AT]] if rag else [AT] * c.M
    M, N, K, n2 = c.M, c.N, c.K, c.N - c.split
    b = {}
    b["x"] = Buf((P, M, K), dev, data=_only_rows(d["x"], at) if not c.part else None)      # merged input: x is never read
    b["W"], b["bias"] = Buf((N, K), dev, data=d["W"]), Buf((N,), dev, data=d["bias"])
    a = _hip.isi_decode_stage_args()
    a.x, a.x_stride, a.W, a.bias = b["x"].ptr, K, b["W"].ptr, b["bias"].ptr
    if c.flags & T.F_LN:
        b["ln_g"], b["ln_b"] = Buf((K,), dev, data=d["ln_g"]), Buf((K,), dev, data=d["ln_b"])
        a.ln_g, a.ln_b = b["ln_g"].ptr, b["ln_b"].ptr
    if c.flags & T.F_RES:
        b["res"] = Buf((P, M, N), dev, data=_only_rows(d["res"], at))
        a.res, a.res_stride, a.res_pos = b["res"].ptr, N, M * N
    if c.flags & T.F_RES_LN:
        b["res_g"], b["res_b"] = Buf((N,), dev, data=d["res_g"]), Buf((N,), dev, data=d["res_b"])
        a.res_g, a.res_b = b["res_g"].ptr, b["res_b"].ptr
    b["out"] = Buf((M, c.split), dev)
    a.out, a.out_stride = b["out"].ptr, c.split
    if c.kv != T.KV_NONE:
        b["out2"] = Buf((P, M, n2), dev) if c.kv == T.KV_F32 else Buf((P, M, n2), dev, torch.int16, SENTINEL16)
        a.out2, a.out2_stride, a.out2_pos = b["out2"].ptr, n2, M * n2
        a.out2_format = _hip.ISI_KV_BF16 if c.kv == T.KV_BF16 else _hip.ISI_KV_F32
    a.split, a.M, a.N, a.K, a.relu, a.eps = c.split, M, N, K, 1 if c.flags & T.F_RELU else 0, EPS
    a.p, a.x_pos = AT, M * K
    if addr in (T.AT_COUNTER, T.AT_ROWS_COUNTER):
        b["counter"] = Buf((4,), dev, torch.int32, POISON32, data=torch.tensor([AT, POISON32, POISON32, POISON32]))
        a.counter = b["counter"].ptr
    if rag:
        b["row_pos"] = Buf(tuple(row_pos.shape), dev, torch.int32, POISON32, data=row_pos)
        a.row_pos = b["row_pos"].ptr
    if c.handoff & T.H_STAT_OUT:
        b["stat_out"] = Buf((M, 2), dev)
        a.stat_out = b["stat_out"].ptr
    if res_stat is not None:
        b["res_stat"] = Buf((M, 2), dev, data=res_stat)
        a.res_stat = b["res_stat"].ptr
    if c.part:
        b["part"] = Buf(tuple(d["part"].shape), dev, data=d["part"])
        a.part, a.part_ns, a.part_hd = b["part"].ptr, c.part[2], c.part[1]
    if c.ws != T.WS_NONE:
        floats = lib.isi_decode_stage_workspace_floats(M, N, K)
        assert floats == 4 + M * -(-K // 512) * N
        b["ws"] = Buf((floats,), dev)
        a.workspace, a.workspace_floats = b["ws"].ptr, floats if c.ws == T.WS_GIVEN else floats - 4 - 1
    with _hip.knob("ISI_DECODE_MFMA_ROWS", c.mfma_rows), _hip.knob("ISI_DECODE_STATS_GLOBAL", c.stats_global):
        rc = lib.isi_decode_stage_ex_f32(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    what = T.decode_stage_case_id(c)
    _settle(rc, what)
    for name, buf in b.items():
        assert buf.pads_intact(), f"{what}: the pads of {name} were written"
    if c.ws == T.WS_SHORT or rc != 0:
        assert "ws" not in b or b["ws"].is_fill(b["ws"].t), f"{what}: a workspace one float short (or a refused call) was written"
    out2 = out2_raw = None
    if c.kv != T.KV_NONE:
        raw = b["out2"].t.cpu()
        mask = torch.zeros(P, M, dtype=torch.bool)
        mask[at, torch.arange(M)] = True
        assert b["out2"].is_fill(raw[~mask]), f"{what}: a k|v slot the case does not address was written"
        out2_raw = raw[at, torch.arange(M)]                           # row m's slot at its position
        out2 = T.bf16_widen(out2_raw) if c.kv == T.KV_BF16 else out2_raw
    stat = b["stat_out"].t.cpu() if "stat_out" in b else None
    return Run(rc, a.kernel, b["out"].t.cpu(), out2, out2_raw, stat, b, at)


def _kwargs(c, d, res_rows, **more):
    kw = dict(bias=d["bias"], ln=(d["ln_g"], d["ln_b"]) if c.flags & T.F_LN else None, res=res_rows if c.flags & T.F_RES else None,
              res_ln=(d["res_g"], d["res_b"]) if c.flags & T.F_RES_LN else None, relu=bool(c.flags & T.F_RELU), eps=EPS, split=c.split)
    kw.update(more)
    return kw


def _expect(c, d, row_pos=None, **more):
    """(spec, float32 yardstick): (out, out2, input statistics) each, for the rows the case addresses."""
    x, res = T.decode_stage_rows(c, d, row_pos)
    x64, x32 = (T.merge_partials_spec(d["part"]), T.merge_partials_f32(d["part"])) if c.part else (x, x)
    kw = _kwargs(c, d, res, **more)
    return T.decode_stage_spec(x64, d["W"], **kw), T.decode_stage_f32(x32, d["W"], **kw)


def _family(c):
    return T.STAGE_FAMILY[c.kernel] + (" (merged input)" if c.part else "")


def _hold_run(c, r, spec, yard, what):
    fam = _family(c)
    _hold(fam, r.out, spec[0], yard[0], f"{what} out")
    if c.kv != T.KV_NONE:
        _hold(fam, r.out2, spec[1], yard[1], f"{what} out2", bf16=c.kv == T.KV_BF16)
    if r.stat is not None:
        _hold(fam, r.stat, spec[2], yard[2], f"{what} stat_out")


@functools.lru_cache(maxsize=None)
def _data(c):
    return T.decode_stage_data(c)


REPORTED = {}


def _run_route_case(c):
    """The case as the table states it, held to the spec; the kernel the library reports goes to REPORTED."""
    cid = T.decode_stage_case_id(c)
    if cid in REPORTED:
        return
    dev = _dev()
    d = _data(c)
    rag = c.addr in (T.AT_ROWS, T.AT_ROWS_COUNTER)
    row_pos = T.decode_stage_row_positions(c.M) if rag else None
    x_rows, res_rows = T.decode_stage_rows(c, d, row_pos)
    res_stat = T.row_stats(res_rows, EPS).float() if c.handoff & T.H_RES_STAT else None
    r = _launch(c, d, dev, row_pos=row_pos, res_stat=res_stat)
    if c.kernel == T.STAGE_REFUSED:
        assert r.rc == -4, (cid, r.rc)
        assert r.bufs["out"].is_fill(r.bufs["out"].t) and ("out2" not in r.bufs or r.bufs["out2"].is_fill(r.bufs["out2"].t)), \
            f"{cid}: a refused call wrote"
    else:
        assert r.rc == 0, (cid, r.rc)
        spec, yard = _expect(c, d, row_pos)
        _hold_run(c, r, spec, yard, cid)
    REPORTED[cid] = r.kernel


@pytest.mark.parametrize("c", T.DECODE_STAGE_CASES, ids=T.decode_stage_case_id)
def test_route_case_against_the_spec(c):
    _run_route_case(c)
    if c.kernel != T.STAGE_REFUSED:
        # a refused call reports the kernel that refused it (the groups-of-8 kernel beyond its LDS) or none (ragged rows)
        assert REPORTED[T.decode_stage_case_id(c)] == c.kernel


HANDOFF_CONSUMERS = [c for c in T.DECODE_STAGE_CASES if c.handoff & T.H_RES_STAT]


@pytest.mark.parametrize("c", HANDOFF_CONSUMERS, ids=T.decode_stage_case_id)
def test_handed_statistics_are_really_read(c):
    """Given deliberately wrong statistics (mean + 0.5, 1 / std x 2) the consumer matches the spec evaluated with THOSE and is
    outside the bound of the plain spec; given the stat_out of a producer that normalised the same rows as its input, it
    matches the plain spec."""
    dev, d = _dev(), _data(c)
    rag = c.addr in (T.AT_ROWS, T.AT_ROWS_COUNTER)
    row_pos = T.decode_stage_row_positions(c.M) if rag else None
    _, res_rows = T.decode_stage_rows(c, d, row_pos)
    true = T.row_stats(res_rows, EPS).float()
    wrong = torch.stack([true[:, 0] + 0.5, true[:, 1] * 2.0], dim=1)
    r = _launch(c, d, dev, row_pos=row_pos, res_stat=wrong)
    assert r.rc == 0
    spec_w, yard_w = _expect(c, d, row_pos, res_stats=wrong)
    spec, yard = _expect(c, d, row_pos)
    fam = _family(c)
    _hold(fam, r.out, spec_w[0], yard_w[0], f"{T.decode_stage_case_id(c)} out, wrong statistics handed")
    with pytest.raises(AssertionError):
        T.compare_rows(r.out, spec[0], yard[0], "the plain spec")
    # the producer: the same rows as the INPUT of a stage of the same row count (K = this stage's N), stat_out on
    prod = T._dsc(T.STAGE_REFUSED, c.M, 8, c.N, flags=T.F_LN, addr=T.AT_VALUE, mfma_rows=c.mfma_rows, handoff=T.H_STAT_OUT)
    pd = T.decode_stage_data(prod, seed=7)
    pd["x"] = torch.zeros(P, c.M, c.N)
    pd["x"][AT] = res_rows
    pr = _launch(prod, pd, dev)
    assert pr.rc == 0 and bool(torch.isfinite(pr.stat).all())
    _hold(T.STAGE_FAMILY[pr.kernel], pr.stat, T.row_stats(res_rows, EPS), T.row_stats(res_rows, EPS, torch.float32), "producer stat_out")
    r = _launch(c, d, dev, row_pos=row_pos, res_stat=pr.stat)
    _hold(fam, r.out, spec[0], yard[0], f"{T.decode_stage_case_id(c)} out, the producer's statistics handed")


def _one_per_instance(cases):
    seen, out = set(), []
    for c in cases:
        k = T.decode_stage_instance(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


POSITION_CASES = _one_per_instance([c for c in T.DECODE_STAGE_CASES if c.kernel != T.STAGE_REFUSED and c.addr == T.AT_VALUE
                                    and c.kv != T.KV_NONE and not c.handoff])


def _bits_equal(x, y):
    if x is None or y is None:
        return x is None and y is None
    as_int = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    return x.dtype == y.dtype and x.shape == y.shape and bool(torch.equal(as_int(x), as_int(y)))


def _same_bits(a, b):
    return all(_bits_equal(x, y) for x, y in ((a.out, b.out), (a.out2_raw, b.out2_raw), (a.stat, b.stat)))


@pytest.mark.parametrize("c", POSITION_CASES, ids=T.decode_stage_case_id)
def test_position_forms_agree(c):
    """By value and by the device counter: one instantiation, the same bits.  row_pos offset to its step and the whole array
    beside the counter: the same bits; with every row at the one position, within the bound of the spec of the launch
    without row_pos (route cases with row_pos put every row at its OWN position and find its k|v in its own slot only)."""
    dev, d = _dev(), _data(c)
    by_value, by_counter = _launch(c, d, dev, addr=T.AT_VALUE), _launch(c, d, dev, addr=T.AT_COUNTER)
    assert by_value.rc == by_counter.rc == 0 and by_value.kernel == by_counter.kernel == c.kernel
    assert _same_bits(by_value, by_counter), "position by value and by the counter differ"
    if c.kernel not in (T.STAGE_ROWS_IN_REGISTERS, T.STAGE_TILES):
        return
    for own in (False, True):
        row_pos = T.decode_stage_row_positions(c.M, own=own)
        direct = _launch(c, d, dev, addr=T.AT_ROWS, row_pos=row_pos)
        beside = _launch(c, d, dev, addr=T.AT_ROWS_COUNTER, row_pos=row_pos)
        assert direct.rc == beside.rc == 0 and direct.kernel == beside.kernel == c.kernel
        assert _same_bits(direct, beside), f"row_pos offset to its step and beside the counter differ (own positions: {own})"
        spec, yard = _expect(c, d, row_pos)
        _hold_run(c, direct, spec, yard, f"{T.decode_stage_case_id(c)} row_pos, {'own positions' if own else 'one position'}")


ROW_CASES = [c for c in T.DECODE_STAGE_CASES if c.kernel in (T.STAGE_ROWS_IN_REGISTERS, T.STAGE_GROUPS_OF_8) and c.M > 1
             and c.addr in (T.AT_VALUE, T.AT_COUNTER) and c.kv in (T.KV_NONE, T.KV_F32) and not c.handoff]


@pytest.mark.parametrize("c", ROW_CASES, ids=T.decode_stage_case_id)
def test_a_row_does_not_depend_on_its_launch(c):
    """GEMV families: row r of an M-row launch against the row alone (the same operations in the same order, up to the compiler's
    contraction): max |difference| <= 4e-6 max |row|."""
    dev, d = _dev(), _data(c)
    batch = _launch(c, d, dev)
    assert batch.rc == 0
    for r_ in (0, c.M - 1):
        c1 = c._replace(M=1)
        d1 = dict(d, x=d["x"][:, r_:r_ + 1].contiguous(), res=d["res"][:, r_:r_ + 1].contiguous())
        alone = _launch(c1, d1, dev)
        assert alone.rc == 0 and alone.kernel in (T.STAGE_ONE_ROW, T.STAGE_GROUPS_OF_8)
        for got, want in ((alone.out[0], batch.out[r_]), (alone.out2[0], batch.out2[r_])) if c.kv else ((alone.out[0], batch.out[r_]),):
            assert float((got - want).abs().max()) <= T.DECODE_STAGE_ROW_INVARIANCE * float(want.abs().max()), (r_, T.decode_stage_case_id(c))


# ---------------------------------------------------------------- single_source_cross_kernel
def _single_source(c, dev, addr, y1, gamma, beta, table, positions):
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    rag = addr in (T.AT_ROWS, T.AT_ROWS_COUNTER)
    p = T.SINGLE_SOURCE_P
    at = [int(v) for v in positions[p]] if rag else [p] * c.B
    masked = torch.full_like(table, float("nan"))
    for m in range(c.B):
        masked[at[m] // c.Cd, 0 if c.shared else m] = table[at[m] // c.Cd, 0 if c.shared else m]
    b = dict(y1=Buf((c.B, c.d), dev, data=y1), g=Buf((c.d,), dev, data=gamma), b=Buf((c.d,), dev, data=beta),
             table=Buf(tuple(table.shape), dev, data=masked), y2=Buf((c.B, c.d), dev))
    a = _hip.isi_decode_single_source_args()
    a.y1, a.ln_g, a.ln_b, a.table, a.y2 = b["y1"].ptr, b["g"].ptr, b["b"].ptr, b["table"].ptr, b["y2"].ptr
    if c.stats:
        b["stat"] = Buf((c.B, 2), dev)
        a.stat_out = b["stat"].ptr
    a.p, a.Cd, a.S_src, a.B, a.d, a.eps = p, c.Cd, T.SINGLE_SOURCE_S_SRC, c.B, c.d, EPS
    a.table_B, a.table_sb = (1, 0) if c.shared else (c.B, 1)
    if addr in (T.AT_COUNTER, T.AT_ROWS_COUNTER):
        b["counter"] = Buf((4,), dev, torch.int32, POISON32, data=torch.tensor([p, POISON32, POISON32, POISON32]))
        a.counter = b["counter"].ptr
    host = positions.contiguous()
    if rag:
        b["row_pos"] = Buf(tuple(positions.shape), dev, torch.int32, POISON32, data=positions)
        a.row_pos, a.row_pos_host = b["row_pos"].ptr, host.data_ptr()
    rc = lib.isi_decode_single_source_f32(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _settle(rc, str(c))
    _hip.check(rc, "isi_decode_single_source_f32")
    for name, buf in b.items():
        assert buf.pads_intact(), f"{c}: the pads of {name} were written"
    return b["y2"].t.cpu(), (b["stat"].t.cpu() if c.stats else None), at


@pytest.mark.parametrize("c", T.SINGLE_SOURCE_CASES, ids=str)
def test_single_source_block_against_the_spec(c):
    dev = _dev()
    g = torch.Generator().manual_seed(31 * c.d + c.B)
    y1 = torch.randn(c.B, c.d, generator=g) * (0.5 + 1.5 * torch.rand(c.B, 1, generator=g)) + torch.randn(c.B, 1, generator=g)
    table = torch.randn(T.SINGLE_SOURCE_S_SRC, 1 if c.shared else c.B, c.d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(c.d, generator=g), 0.1 * torch.randn(c.d, generator=g)
    positions = T.single_source_positions(c)
    y2, stat, at = _single_source(c, dev, c.addr, y1, gamma, beta, table, positions)
    spec, yard = (f(y1, gamma, beta, table, at, c.Cd, EPS) for f in (T.single_source_spec, T.single_source_f32))
    _hold("single_source", y2, spec[0], yard[0], f"{c} y2")
    if c.stats:
        _hold("single_source", stat, spec[1], yard[1], f"{c} stat_out")
    # the other form of the same addressing: the same bits
    sibling = {T.AT_VALUE: T.AT_COUNTER, T.AT_COUNTER: T.AT_VALUE, T.AT_ROWS: T.AT_ROWS_COUNTER, T.AT_ROWS_COUNTER: T.AT_ROWS}[c.addr]
    y2s, stats, _ = _single_source(c, dev, sibling, y1, gamma, beta, table, positions)
    assert _bits_equal(y2, y2s) and _bits_equal(stat, stats)
    # row_pos with every row at the one position: the spec of the launch without row_pos
    if c.addr in (T.AT_VALUE, T.AT_COUNTER):
        y2r, statr, _ = _single_source(c, dev, T.AT_ROWS, y1, gamma, beta, table, T.single_source_positions(c, own=False))
        _hold("single_source", y2r, spec[0], yard[0], f"{c} y2, row_pos at one position")
        if c.stats:
            _hold("single_source", statr, spec[1], yard[1], f"{c} stat_out, row_pos at one position")


# ---------------------------------------------------------------- last: what ran
def test_every_route_ran_as_the_table_states():
    """The kernel the library REPORTS for every case is the one the table states, and the cases whose report agrees cover every
    family and every template instantiation the launchers can pick (T.decode_stage_coverage_gaps): a route added to
    stage_kernel() or to a launcher without a case here fails this test."""
    for c in T.DECODE_STAGE_CASES:
        _run_route_case(c)
    wrong = [(T.decode_stage_case_id(c), REPORTED[T.decode_stage_case_id(c)]) for c in T.DECODE_STAGE_CASES
             if c.kernel != T.STAGE_REFUSED and REPORTED[T.decode_stage_case_id(c)] != c.kernel]
    assert wrong == []
    assert {REPORTED[T.decode_stage_case_id(c)] for c in T.DECODE_STAGE_CASES if c.kernel == T.STAGE_REFUSED} == {T.STAGE_GROUPS_OF_8, T.STAGE_REFUSED}
    assert T.decode_stage_coverage_gaps([c for c in T.DECODE_STAGE_CASES if REPORTED[T.decode_stage_case_id(c)] == c.kernel]) == []
    assert {T.STAGE_FAMILY[c.kernel] for c in T.DECODE_STAGE_CASES} == set(T.STAGE_FAMILY.values())
