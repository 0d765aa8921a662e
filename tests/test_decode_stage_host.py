"""The float64 specifications of the decoding loop's stage kernels (tests/tests_support.py), held on the host: each equals an
independent float64 torch computation, its float32 evaluation (the yardstick of tests/test_decode_stage_gpu.py) passes
`compare_rows`, and every mutant -- a way the kernels of csrc/prior_decode.hip could be subtly wrong -- falls outside the
bound.  Also without a GPU: the refusals of isi_decode_stage_ex_f32 and isi_decode_single_source_f32, and that the route table
is the list of `stagex/` cases tests/decode_plan_tracer.cpp pins (tests/decode_plan_trace.txt), kernel for kernel."""
import ctypes as C
import pathlib

import pytest
import torch
import torch.nn.functional as F

import tests_support as T

ROOT = pathlib.Path(__file__).resolve().parent.parent
EPS = 1e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _stage(M=5, N=40, K=100, seed=1, P=T.DECODE_STAGE_P):
    c = T._dsc(T.STAGE_ROWS_IN_REGISTERS, M, N, K, 7, 15, T.KV_F32)
    d = T.decode_stage_data(c, seed)
    kw = dict(bias=d["bias"], ln=(d["ln_g"], d["ln_b"]), res=d["res"][P], res_ln=(d["res_g"], d["res_b"]), relu=True, eps=EPS, split=7)
    return c, d, d["x"][P], kw


def _hold(got, spec, yard, what="mutant"):
    """compare_rows on out, out2 and (where both have them) the statistics."""
    return [T.compare_rows(g, s, y, f"{what}[{i}]") for i, (g, s, y) in enumerate(zip(got, spec, yard)) if s is not None and g is not None]


# ---------------------------------------------------------------- the specs against float64 torch
@pytest.mark.parametrize("M,N,K,flags", [(1, 40, 64, 15), (5, 24, 100, 7), (3, 516, 512, 6), (9, 24, 2560, 9), (33, 48, 520, 0)])
def test_stage_spec_equals_float64_torch(M, N, K, flags):
    c = T._dsc(T.STAGE_TILES, M, N, K, 7, flags, T.KV_F32)
    d = T.decode_stage_data(c)
    x, res = d["x"][1].double(), d["res"][1].double()
    xn = F.layer_norm(x, (K,), d["ln_g"].double(), d["ln_b"].double(), EPS) if flags & T.F_LN else x
    y = xn @ d["W"].double().t() + d["bias"].double()
    if flags & T.F_RES:
        y = y + (F.layer_norm(res, (N,), d["res_g"].double(), d["res_b"].double(), EPS) if flags & T.F_RES_LN else res)
    if flags & T.F_RELU:
        y = torch.relu(y)
    out, out2, stats = T.decode_stage_spec(d["x"][1], d["W"], d["bias"], (d["ln_g"], d["ln_b"]) if flags & T.F_LN else None,
                                           d["res"][1] if flags & T.F_RES else None,
                                           (d["res_g"], d["res_b"]) if flags & T.F_RES_LN else None, bool(flags & T.F_RELU), EPS, 7)
    assert out.dtype == torch.float64 and out.shape == (M, 7) and out2.shape == (M, N - 7)
    torch.testing.assert_close(torch.cat([out, out2], dim=1), y, rtol=1e-12, atol=1e-12)
    if flags & T.F_LN:
        var = x.var(dim=1, unbiased=False)
        torch.testing.assert_close(stats, torch.stack([x.mean(dim=1), (var + EPS).rsqrt()], dim=1), rtol=1e-12, atol=1e-12)
    else:
        assert stats is None
    if flags & T.F_RES_LN:       # the residual's statistics as given = the statistics formed from the rows
        given = T.decode_stage_spec(d["x"][1], d["W"], d["bias"], (d["ln_g"], d["ln_b"]) if flags & T.F_LN else None, d["res"][1],
                                    (d["res_g"], d["res_b"]), bool(flags & T.F_RELU), EPS, 7, res_stats=T.row_stats(d["res"][1], EPS))
        torch.testing.assert_close(given[0], out, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(given[1], out2, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("part", [(4, 16, 1, 0), (8, 32, 2, 1), (4, 64, 8, 2), (16, 32, 8, 0), (8, 64, 3, 1)])
def test_merge_spec_equals_float64_torch(part):
    """Independent form: a split holds o_s = sum_j exp(l_j - m_s) v_j / 1 and sum_s = sum_j exp(l_j - m_s), so the merged row is
    sum_s softmax_s(m_s + log sum_s) o_s / sum_s ... written with logsumexp, no explicit maximum."""
    H, HD, NS, _ = part
    d = T.decode_stage_data(T._dsc(T.STAGE_ONE_ROW, 1, 40, H * HD, flags=6, part=part))
    p = d["part"].double()
    o, m, l = p[:, :, :HD], p[:, :, HD], p[:, :, HD + 1]
    total = torch.logsumexp(m + torch.log(l), dim=1, keepdim=True)         # log of the whole softmax denominator
    want = (torch.exp(m - total).unsqueeze(-1) * o).sum(dim=1).reshape(1, -1)
    got = T.merge_partials_spec(d["part"])
    assert got.shape == (1, H * HD) and bool(torch.isfinite(got).all())
    torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("c", T.SINGLE_SOURCE_CASES[:8], ids=str)
def test_single_source_spec_equals_float64_torch(c):
    g = _gen(c.d + c.B)
    y1, table = torch.randn(c.B, c.d, generator=g), torch.randn(T.SINGLE_SOURCE_S_SRC, 1 if c.shared else c.B, c.d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(c.d, generator=g), 0.1 * torch.randn(c.d, generator=g)
    pos = T.single_source_positions(c)[T.SINGLE_SOURCE_P]
    want = F.layer_norm(y1.double(), (c.d,), gamma.double(), beta.double(), EPS)
    for m in range(c.B):
        want[m] += table[int(pos[m]) // c.Cd, 0 if c.shared else m].double()
    y2, stats = T.single_source_spec(y1, gamma, beta, table, pos, c.Cd, EPS)
    torch.testing.assert_close(y2, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(stats[:, 0], want.mean(dim=1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(stats[:, 1], (want.var(dim=1, unbiased=False) + EPS).rsqrt(), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- the yardsticks pass, the mutants do not
def test_float32_yardsticks_pass():
    for M, N, K in ((5, 40, 100), (3, 24, 2560), (33, 48, 520)):
        _, d, x, kw = _stage(M, N, K)
        spec, yard = T.decode_stage_spec(x, d["W"], **kw), T.decode_stage_f32(x, d["W"], **kw)
        assert all(r.ratio <= 1.0 for r in _hold(yard, spec, yard, "yardstick")) and yard[0].dtype == torch.float32
    for part in ((8, 32, 2, 1), (4, 64, 8, 2), (16, 32, 8, 0)):
        d = T.decode_stage_data(T._dsc(T.STAGE_ONE_ROW, 1, 40, part[0] * part[1], flags=6, part=part))
        T.compare_rows(T.merge_partials_f32(d["part"]), T.merge_partials_spec(d["part"]), T.merge_partials_f32(d["part"]), "merge")
    c = T.SINGLE_SOURCE_CASES[7]
    g = _gen(3)
    y1, table = torch.randn(c.B, c.d, generator=g), torch.randn(T.SINGLE_SOURCE_S_SRC, c.B, c.d, generator=g)
    pos = T.single_source_positions(c)[T.SINGLE_SOURCE_P]
    a = (y1, torch.ones(c.d), torch.zeros(c.d), table, pos, c.Cd, EPS)
    _hold(T.single_source_f32(*a), T.single_source_spec(*a), T.single_source_f32(*a), "single-source")
    # bf16: the value rounded to nearest-even passes
    _, d, x, kw = _stage()
    spec, yard = T.decode_stage_spec(x, d["W"], **kw), T.decode_stage_f32(x, d["W"], **kw)
    r = T.compare_rows_bf16(T.bf16_widen(T.bf16_bits(yard[1])), spec[1], yard[1], "bf16")
    assert r.ratio <= 1.5 and r.err > 2.0 ** -12             # (the stored value really is 8 bits wide)


def _rejected(got, spec, yard):
    with pytest.raises(AssertionError, match="times the float32 yardstick|not finite"):
        _hold(got, spec, yard)


def test_mutant_out2_columns_shifted_by_one():
    _, d, x, kw = _stage()
    spec, yard = T.decode_stage_spec(x, d["W"], **kw), T.decode_stage_f32(x, d["W"], **kw)
    mutant = T.decode_stage_f32(x, d["W"], out2_shift=1, **kw)
    T.compare_rows(mutant[0], spec[0], yard[0], "out is untouched")
    _rejected(mutant[1:2], spec[1:2], yard[1:2])


@pytest.mark.parametrize("which", ["stat_perm", "res_stat_perm"])
def test_mutant_a_row_takes_its_neighbours_statistics(which):
    _, d, x, kw = _stage()
    spec, yard = T.decode_stage_spec(x, d["W"], **kw), T.decode_stage_f32(x, d["W"], **kw)
    mutant = T.decode_stage_f32(x, d["W"], **{which: torch.arange(5).roll(1)}, **kw)
    _rejected(mutant[:1], spec[:1], yard[:1])
    _rejected(mutant[1:2], spec[1:2], yard[1:2])


def test_mutant_variance_over_a_width_padded_to_64():
    _, d, x, kw = _stage(K=100, N=40)
    spec, yard = T.decode_stage_spec(x, d["W"], **kw), T.decode_stage_f32(x, d["W"], **kw)
    mutant = T.decode_stage_f32(x, d["W"], pad_to=64, **kw)
    _rejected(mutant[:1], spec[:1], yard[:1])
    _rejected(mutant[2:], spec[2:], yard[2:])                 # the statistics themselves
    # a width that is a multiple of 64 has no such lanes: the mutant is the yardstick there
    _, d, x, kw = _stage(K=128, N=64)
    assert torch.equal(T.decode_stage_f32(x, d["W"], pad_to=64, **kw)[0], T.decode_stage_f32(x, d["W"], **kw)[0])


def test_mutant_merge_leaves_out_the_last_split():
    d = T.decode_stage_data(T._dsc(T.STAGE_ONE_ROW, 1, 40, 256, flags=6, part=(8, 32, 3, 0)))
    spec, yard = T.merge_partials_spec(d["part"]), T.merge_partials_f32(d["part"])
    _rejected([T.merge_partials_f32(d["part"], splits=2)], [spec], [yard])


def test_mutant_merge_without_the_maximum_subtraction():
    d = T.decode_stage_data(T._dsc(T.STAGE_ONE_ROW, 1, 40, 256, flags=6, part=(4, 64, 8, 2)))
    part = d["part"].clone()
    part[:, :, 64] += 95.0 - part[:, :, 64].amax()            # maxima up to 95 and one 60 below: exp(95) is beyond float32
    spec, yard = T.merge_partials_spec(part), T.merge_partials_f32(part)
    T.compare_rows(yard, spec, yard, "with the subtraction")
    _rejected([T.merge_partials_f32(part, subtract_max=False)], [spec], [yard])


def test_mutant_k_tail_beyond_2048_dropped():
    _, d, x, kw = _stage(M=3, N=24, K=2560)
    spec, yard = T.decode_stage_spec(x, d["W"], **kw), T.decode_stage_f32(x, d["W"], **kw)
    mutant = T.decode_stage_f32(x, d["W"], k_keep=2048, **kw)
    _rejected(mutant[:1], spec[:1], yard[:1])
    _rejected(mutant[1:2], spec[1:2], yard[1:2])


def test_mutant_bf16_store_truncates():
    _, d, x, kw = _stage()
    spec, yard = T.decode_stage_spec(x, d["W"], **kw), T.decode_stage_f32(x, d["W"], **kw)
    with pytest.raises(AssertionError, match="beyond half a bf16 ulp"):
        T.compare_rows_bf16(T.bf16_widen(T.bf16_bits(yard[1], truncate=True)), spec[1], yard[1], "truncated")


def test_mutant_ragged_launch_reads_every_row_at_row_0s_position():
    c, d, _, kw = _stage()
    row_pos = T.decode_stage_row_positions(c.M)
    x, res = T.decode_stage_rows(c, d, row_pos)
    kw["res"] = res
    spec, yard = T.decode_stage_spec(x, d["W"], **kw), T.decode_stage_f32(x, d["W"], **kw)
    assert len(set(row_pos[T.DECODE_STAGE_P].tolist())) == T.DECODE_STAGE_POSITIONS       # rows really stand apart
    x0, res0 = T.decode_stage_rows(c, d, row_pos[:, :1].expand(-1, c.M))
    kw0 = dict(kw, res=res0)
    mutant = T.decode_stage_f32(x0, d["W"], **kw0)
    _rejected(mutant[:1], spec[:1], yard[:1])
    _rejected(mutant[2:], spec[2:], yard[2:])


# ---------------------------------------------------------------- refusals, no GPU
FAKE = 0x10000      # non-null, 16-byte aligned, never dereferenced on the host


def _args(M=2, N=24, K=64, **kw):
    from interactive_spectrogram_inpainting import _hip
    a = _hip.isi_decode_stage_args()
    a.x, a.x_stride, a.W, a.bias, a.out, a.out_stride = FAKE, K, FAKE, FAKE, FAKE, N
    a.split, a.M, a.N, a.K, a.eps, a.p = N, M, N, K, EPS, 1
    a.x_pos = M * K
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refused(a, code, word):
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    assert lib.isi_decode_stage_ex_f32(C.byref(a), None) == code
    assert word.encode() in lib.isi_last_error(), lib.isi_last_error()
    return a.kernel


def test_stage_entry_refuses_on_the_host():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    INVALID, UNSUPPORTED = -1, -4
    assert lib.isi_decode_stage_ex_f32(None, None) == INVALID
    _refused(_args(x=None), INVALID, "bad argument")
    _refused(_args(M=257), INVALID, "bad argument")
    _refused(_args(K=66), INVALID, "multiples of 4")
    _refused(_args(x=FAKE + 4), INVALID, "16-byte aligned")
    _refused(_args(x_pos=66), INVALID, "x_pos")
    _refused(_args(ln_g=FAKE), INVALID, "come together")
    _refused(_args(res_g=FAKE, res_b=FAKE), INVALID, "with a residual")
    _refused(_args(ln_g=FAKE + 4, ln_b=FAKE), INVALID, "ln_g")
    _refused(_args(out2=FAKE), INVALID, "split")                                   # out2 without a split
    _refused(_args(split=7), INVALID, "split")                                     # a split without out2
    _refused(_args(out2=FAKE, split=7, out2_format=2), INVALID, "out2_format")
    _refused(_args(out2=FAKE + 8, split=7, out2_format=_hip.ISI_KV_BF16), INVALID, "bf16 out2")
    _refused(_args(x_pos=0, counter=FAKE), INVALID, "counter")
    _refused(_args(x_pos=0, row_pos=FAKE), INVALID, "row_pos")
    _refused(_args(res_pos=48), INVALID, "res_pos")
    _refused(_args(stat_out=FAKE), INVALID, "stat_out")                            # nothing forms them without ln_g
    _refused(_args(res=FAKE, res_stride=24, res_stat=FAKE), INVALID, "res_stat")
    _refused(_args(M=1, part=FAKE, part_ns=9, part_hd=16), INVALID, "part")
    _refused(_args(M=1, part=FAKE, part_ns=2, part_hd=16, ln_g=FAKE, ln_b=FAKE), INVALID, "part")
    # what the chosen kernel would silently ignore
    ln = dict(ln_g=FAKE, ln_b=FAKE)
    rs = dict(res=FAKE, res_stride=24, res_g=FAKE, res_b=FAKE)
    assert _refused(_args(K=2052, stat_out=FAKE, **ln), UNSUPPORTED, "stat_out") == _hip.ISI_STAGE_GROUPS_OF_8
    assert _refused(_args(K=2052, res_stat=FAKE, **rs), UNSUPPORTED, "res_stat") == _hip.ISI_STAGE_GROUPS_OF_8
    assert _refused(_args(M=1, K=1024, part=FAKE, part_ns=2, part_hd=64), UNSUPPORTED, "part") == _hip.ISI_STAGE_ROWS_IN_REGISTERS
    assert _refused(_args(M=2, K=256, part=FAKE, part_ns=2, part_hd=64), UNSUPPORTED, "part") == _hip.ISI_STAGE_ROWS_IN_REGISTERS
    assert _refused(_args(M=1, K=2052, part=FAKE, part_ns=2, part_hd=4), UNSUPPORTED, "part") == _hip.ISI_STAGE_GROUPS_OF_8
    # the plan's own refusals
    assert _refused(_args(M=3, K=2052, row_pos=FAKE), UNSUPPORTED, "ragged rows") == _hip.ISI_STAGE_REFUSED
    assert _refused(_args(M=8, K=5120), UNSUPPORTED, "LDS") == _hip.ISI_STAGE_GROUPS_OF_8
    # isi_decode_stage_f32 is as it was: its two refusals the new entry lifts
    assert lib.isi_decode_stage_f32(FAKE, 2052, None, None, FAKE, None, None, 0, None, None, FAKE, 24, 2, 24, 2052, 0, EPS, None, 0, None) == -4
    assert b"K <= 2048" in lib.isi_last_error()
    assert lib.isi_decode_stage_f32(FAKE, 64, None, None, FAKE, None, FAKE, 516, FAKE, FAKE, FAKE, 516, 2, 516, 64, 0, EPS, None, 0, None) == -4
    assert b"at most 512 features" in lib.isi_last_error()


def test_single_source_entry_refuses_on_the_host():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()

    def call(**kw):
        a = _hip.isi_decode_single_source_args()
        a.y1 = a.ln_g = a.ln_b = a.table = a.y2 = FAKE
        a.p, a.Cd, a.S_src, a.B, a.d, a.eps, a.table_B, a.table_sb = 5, 4, 2, 3, 64, EPS, 3, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.isi_decode_single_source_f32(C.byref(a), None), lib.isi_last_error()

    assert lib.isi_decode_single_source_f32(None, None) == -1
    assert call(table=None)[0] == -1
    rc, msg = call(d=1028)
    assert rc == -4 and b"d <= 1024" in msg
    rc, msg = call(Cd=0)
    assert rc == -1 and b"Cd >= 1" in msg
    rc, msg = call(p=8)                                      # 8 // 4 = 2 = S_src
    assert rc == -1 and b"without a source row" in msg
    rc, msg = call(table_B=2)
    assert rc == -1 and b"table_B" in msg
    rc, msg = call(row_pos=FAKE)
    assert rc == -1 and b"row_pos_host" in msg
    host = (C.c_int32 * 18)(*([0] * 15 + [1, 9, 2]))         # step 5: row 1 stands at 9, 9 // 4 >= S_src
    rc, msg = call(row_pos=FAKE, row_pos_host=C.cast(host, C.c_void_p).value)
    assert rc == -1 and b"without a source row" in msg


# ---------------------------------------------------------------- the route table and the tracer's cases are one list
def test_route_table_is_the_tracers_case_list():
    lines = [l.split() for l in (ROOT / "tests" / "decode_plan_trace.txt").read_text().splitlines() if l.startswith("stagex/")]
    traced = {l[0]: (int(l[1]), l[4]) for l in lines}
    table = {T.decode_stage_case_id(c): c for c in T.DECODE_STAGE_CASES}
    assert len(table) == len(T.DECODE_STAGE_CASES) == len(lines) and set(table) == set(traced)
    for cid, c in table.items():
        rc, kinds = traced[cid]
        if c.kernel == T.STAGE_REFUSED:
            assert (rc, kinds) == (-4, "-"), cid
            continue
        inst = T.decode_stage_instance(c)
        launches = len(inst[1]) if c.kernel == T.STAGE_GROUPS_OF_8 else 1
        assert (rc, kinds) == (0, f"{T.STAGE_LAUNCHER[c.kernel]}:{launches}"), cid


def test_route_table_covers_every_instantiation():
    """Every template instantiation the launchers of csrc/prior_decode.hip can pick (the GPU file asserts the same of the
    kernels the library REPORTS; this is the table's own claim, checkable without a GPU)."""
    assert T.decode_stage_coverage_gaps(T.DECODE_STAGE_CASES) == []
    # ... and the check has teeth: without the bf16 cases, or without the ragged ones, it names what is missing
    assert T.decode_stage_coverage_gaps([c for c in T.DECODE_STAGE_CASES if c.kv != T.KV_BF16])
    assert T.decode_stage_coverage_gaps([c for c in T.DECODE_STAGE_CASES if c.addr < T.AT_ROWS])
    assert ("row_gemvm", 8, 2, True, True) in T.decode_stage_coverage_gaps([c for c in T.DECODE_STAGE_CASES if c.K <= 1024])
    ss = T.SINGLE_SOURCE_CASES
    assert {c.d for c in ss} == {64, 100, 1024} and {c.B for c in ss} == {1, 3, 4, 5} and {c.Cd for c in ss} == {1, 4}
    assert {(c.shared, c.addr in (T.AT_ROWS, T.AT_ROWS_COUNTER)) for c in ss} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c.addr for c in ss} == {0, 1, 2, 3} and {c.stats for c in ss} == {False, True}
