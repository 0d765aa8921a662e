"""The small kernels of the VQ-VAE training step against the float64 specifications of tests/tests_support.py, through the
C-ABI: relu_bwd_kernel, axpy_kernel, vq_bwd_kernel, vq_bwd_rows_kernel, add_gate_rows_kernel, colsum_flat_kernel and
colsum_partial_kernel with reduce_rows_kernel, the three MSE kernels, vq_ema_update_kernel and pad_channels4_kernel of
csrc/train_ops.hip, vq_finalize_kernel and embed_code_kernel of csrc/vq_nearest.hip, the pair conversion and relu_inplace
of csrc/pack.hip -- at the smallest shapes where each can go wrong: every vector tail, every route of colsum_f32, row
strides wider than the row, K above the EMA update's 1024 threads, and one length past the cap of every grid-stride launch
(test functions of their own: they hold up to four 34 MB operands).

Every input and output is a view inside a buffer of NaN whose guards (in front, behind, between the row width and the row
stride) must keep their bits; workspaces have exactly the size the C-ABI asks for and start as NaN; in-place operands are
compared with the spec of their original contents.  Operations that round nowhere are held bit for bit (relu_bwd,
add_gate_rows without a second term, embed_code, the pair round trip, relu_inplace, pad_channels4); everything else goes
through `tests_support.compare_rows` with the float32 torch evaluation as yardstick, margin 8, floor 2^-23, two-dimensional
operands as [M, C] rows.  tests/test_train_ops_host.py shows, without a GPU, what the comparisons reject, and holds the
argument refusals: no test here passes a pointer a kernel could not take.

A recording aid, not a check: with ISI_TRAIN_OPS_RECORD=<file> in the environment every comparison's error, yardstick and
ratio are written there when the module ends, the worst ratio first (profiles/train_ops_checks.txt is such a run on an
MI355X: the worst ratio there is 4.01, colsum_flat_kernel at M = 70 000, C = 1; 3.78 at M = 65 536, C = 2; every other
comparison stays below 2.2)."""
import ctypes as C
import os

import pytest
import torch

import tests_support as TS
from test_prior_gpu import _dev
from test_prior_row_ops_gpu import PAD, Guarded, _assert_guards, _vec

pytestmark = pytest.mark.gpu

CAP = TS.TRAIN_OPS_GRID_CAP    # threads of `grid_for`'s largest launch (8192 blocks); pair conversion: the same count of groups
RECORD = []                    # RowCheck of every comparison of this process (bit-for-bit ones with error and ratio 0)
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_TRAIN_OPS_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# kernel error, float32-torch yardstick (floored at 2^-23) and their ratio against the float64 spec, per comparison of\n"
                f"# tests/test_train_ops_gpu.py; metric and bound: tests_support.compare_rows (ratio <= {TS.ROW_OPS_MARGIN:g}).  Worst ratio first;\n"
                "# 'exact': held bit for bit, no ratio.\n")
        for c in sorted(RECORD, key=lambda r: -r.ratio):
            if c.yardstick == 0.0:
                f.write(f"   exact  {c.what}\n")
            else:
                f.write(f"{c.ratio:8.3f}  err {c.err:.3e}  yardstick {c.yardstick:.3e}  {c.what}\n")


def _check(case, got, ref, yardstick, what):
    got = got.detach().cpu()
    err, yard = TS.row_error(got, ref), max(TS.row_error(yardstick, ref), TS.ROW_OPS_FLOOR)
    print(f"{case} {what}: err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    RECORD.append(TS.RowCheck(f"{case} {what}", err, yard, err / yard))                  # (recorded whether it passes or not)
    TS.compare_rows(got, ref, yardstick, f"{case} {what}")


def _exact(case, got, want, what):
    assert TS.same_bits(got, want), f"{case} {what}: not the spec's bits"
    RECORD.append(TS.RowCheck(f"{case} {what}", 0.0, 0.0, 0.0))


def _lib():
    from interactive_spectrogram_inpainting import _hip
    return _hip.lib(), _dev()


def _run(L, rc):
    assert rc == 0, L.isi_last_error()
    torch.cuda.synchronize()


def _unchanged(case, **inputs):
    for name, (g, src) in inputs.items():
        assert TS.same_bits(g.view.reshape(src.shape), src), f"{case}: the kernel changed its input {name}"


class IntGuarded:
    """An integer vector inside a buffer of `poison` (no NaN among integers), PAD elements on either side."""

    def __init__(self, values, dev, poison):
        n = values.numel()
        self.buf = torch.full((PAD + n + PAD,), poison, dtype=values.dtype, device=dev)
        self.buf[PAD:PAD + n] = values.to(dev)
        self.before = self.buf.clone()
        self.ptr = self.buf[PAD:].data_ptr()

    def intact(self):
        return bool(torch.equal(self.buf, self.before))


def _release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- relu_bwd
def _relu_bwd_case(n):
    L, dev = _lib()
    case = f"relu_bwd n={n}"
    dy, y = TS.gate_data(n, torch.Generator().manual_seed(1000 + n % 9973))
    gdy, gy = _vec(n, dev, dy), _vec(n, dev, y)
    _run(L, L.isi_relu_bwd_f32(gdy.ptr, gy.ptr, n, None))
    _assert_guards(case, dy=gdy, y=gy)
    _unchanged(case, y=(gy, y))
    _exact(case, gdy.view.reshape(n), TS.relu_bwd_spec(dy, y), "dy")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025])
def test_relu_bwd_bit_for_bit(n):
    _relu_bwd_case(n)


def test_relu_bwd_past_the_grid_cap():
    _relu_bwd_case(4 * CAP + 1203)                        # second pass of the loop, then a tail of 3
    _release()


# ------------------------------------------------------------------------------------------------------- axpy and vq_bwd
def _axpy_case(n, alpha):
    L, dev = _lib()
    case = f"axpy n={n} alpha={alpha}"
    gen = torch.Generator().manual_seed(1100 + n % 9973)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ga, gb = _vec(n, dev, a), _vec(n, dev, b)
    _run(L, L.isi_axpy_f32(ga.ptr, gb.ptr, alpha, n, None))
    _assert_guards(case, a=ga, b=gb)
    _unchanged(case, b=(gb, b))
    _check(case, ga.view.reshape(n), TS.axpy_spec(a, b, alpha), TS.axpy_f32(a, b, alpha), "a")


@pytest.mark.parametrize("alpha", [1.0, -0.5])
@pytest.mark.parametrize("n", [4, 8, 1020, 1024, 1028])
def test_axpy_against_float64(n, alpha):
    _axpy_case(n, alpha)


def test_axpy_past_the_grid_cap():
    _axpy_case(4 * CAP + 1200, -0.5)
    _release()


def _vq_bwd_case(n, g):
    L, dev = _lib()
    case = f"vq_bwd n={n} g_diff={g}"
    gen = torch.Generator().manual_seed(1200 + n % 9973)
    dq, z, q_st = (torch.randn(n, generator=gen) for _ in range(3))
    gdq, gz, gq, gg = _vec(n, dev, dq), _vec(n, dev, z), _vec(n, dev, q_st), _vec(1, dev, torch.tensor([g]))
    dz = _vec(n, dev)
    _run(L, L.isi_vq_bwd_f32(dz.ptr, gdq.ptr, gz.ptr, gq.ptr, gg.ptr, n, None))
    _assert_guards(case, dz=dz, dq=gdq, z=gz, q_st=gq, g_diff=gg)
    _unchanged(case, dq=(gdq, dq), z=(gz, z), q_st=(gq, q_st))
    _check(case, dz.view.reshape(n), TS.vq_bwd_spec(dq, z, q_st, g), TS.vq_bwd_f32(dq, z, q_st, g), "dz")


@pytest.mark.parametrize("g", [0.25, 0.0])
@pytest.mark.parametrize("n", [4, 8, 1020, 1024, 1028])
def test_vq_bwd_against_float64(n, g):
    _vq_bwd_case(n, g)


def test_vq_bwd_past_the_grid_cap():
    _vq_bwd_case(4 * CAP + 1200, 0.25)
    _release()


# --------------------------------------------------------------------------------------- vq_bwd_rows and add_gate_rows
ROW_SHAPES = [(1, 4, 4), (3, 8, 12), (257, 64, 128), (5, 128, 192)]      # (M, C, row stride of the strided operand)
ROW_SHAPE_PAST_CAP = (65600, 128, 192)                                    # 2 099 200 float4 against 2 097 152 threads


def _vq_bwd_rows_case(M, D, ld, g):
    L, dev = _lib()
    case = f"vq_bwd_rows M={M} D={D} ldq={ld} g_diff={g}"
    gen = torch.Generator().manual_seed(1300 + M + D)
    dq, z, q_st = (torch.randn(M, D, generator=gen) for _ in range(3))
    gdq = Guarded(M, D, ld, dev, dq)                      # NaN between the row's end and the next row
    gz, gq, gg = Guarded(M, D, D, dev, z), Guarded(M, D, D, dev, q_st), _vec(1, dev, torch.tensor([g]))
    dz = Guarded(M, D, D, dev)
    _run(L, L.isi_vq_bwd_rows_f32(dz.ptr, gdq.ptr, ld, gz.ptr, gq.ptr, gg.ptr, M, D, None))
    _assert_guards(case, dz=dz, dq=gdq, z=gz, q_st=gq, g_diff=gg)
    _check(case, dz.view, TS.vq_bwd_spec(dq, z, q_st, g), TS.vq_bwd_f32(dq, z, q_st, g), "dz")


@pytest.mark.parametrize("g", [0.25, 0.0])
@pytest.mark.parametrize("M,D,ld", ROW_SHAPES)
def test_vq_bwd_rows_against_float64(M, D, ld, g):
    _vq_bwd_rows_case(M, D, ld, g)


def test_vq_bwd_rows_past_the_grid_cap():
    _vq_bwd_rows_case(*ROW_SHAPE_PAST_CAP, 0.25)
    _release()


def _add_gate_rows_case(M, Cc, ld):
    """All four forms on one set of operands: b and y, b only, y only, neither.  The gated forms read an `a` with NaN and
    +-inf at the masked places (a selection must not let them through); the ungated forms read a finite one."""
    L, dev = _lib()
    gen = torch.Generator().manual_seed(1400 + M + Cc)
    a_gated, y = (t.reshape(M, Cc) for t in TS.gate_data(M * Cc, gen))
    a_plain, b = torch.randn(M, Cc, generator=gen), torch.randn(M, Cc, generator=gen)
    ga_gated, ga_plain = Guarded(M, Cc, ld, dev, a_gated), Guarded(M, Cc, ld, dev, a_plain)
    gb, gy = Guarded(M, Cc, Cc, dev, b), Guarded(M, Cc, Cc, dev, y)
    for with_b, with_y in ((True, True), (True, False), (False, True), (False, False)):
        case = f"add_gate_rows M={M} C={Cc} lda={ld} b={int(with_b)} y={int(with_y)}"
        a, ga = (a_gated, ga_gated) if with_y else (a_plain, ga_plain)
        out = Guarded(M, Cc, Cc, dev)
        _run(L, L.isi_add_gate_rows_f32(out.ptr, ga.ptr, ld, gb.ptr if with_b else None, gy.ptr if with_y else None, M, Cc, None))
        _assert_guards(case, out=out, a=ga, b=gb, y=gy)
        bb, yy = b if with_b else None, y if with_y else None
        if with_b:
            _check(case, out.view, TS.add_gate_rows_spec(a, bb, yy), TS.add_gate_rows_f32(a, bb, yy), "out")
        else:
            _exact(case, out.view, TS.add_gate_rows_spec(a, bb, yy), "out")
        del out


@pytest.mark.parametrize("M,Cc,ld", ROW_SHAPES)
def test_add_gate_rows_against_float64(M, Cc, ld):
    _add_gate_rows_case(M, Cc, ld)


def test_add_gate_rows_past_the_grid_cap():
    _add_gate_rows_case(*ROW_SHAPE_PAST_CAP)
    _release()


# --------------------------------------------------------------------------------------------------------------- colsum
# (M, C, layout, data, route).  layout: "dense"; "strided" (x_stride = C + 64, NaN between the rows); "offset" (dense, 4 bytes
# past a 16-byte boundary: the float4 route is refused and the scalar one, for which this is aligned, runs).  route: what
# colsum_f32 chooses, asserted from its own conditions (tests_support.colsum_route).  M: 1, 3, 4 inside one block; 255, 256,
# 257 around one block's 256 rows (partial: 64 rows per thread, the four-way unroll and its remainder); 65 536 = 256 blocks
# of 256 rows, the last M at the cap; 65 537, 70 000, 70 001 past it (a block's share is 257 / 274 rows; flat: 70 000 floats
# fill 69 of 256 blocks, the others must write zeros over their NaN).  C: 1, 2 take the flat kernel's C < 4 fold, 3 and 1025
# are no powers of two, 1025 = 17 trips over 64 columns with one column in the last, 2048 > 1024.
COLSUM_CASES = [
    (4, 1, "dense", "randn", "flat"), (3, 1, "dense", "offset", "partial"), (65536, 1, "dense", "offset", "flat"),
    (70001, 1, "dense", "randn", "partial"), (70000, 1, "dense", "randn", "flat"), (255, 1, "strided", "randn", "partial"),
    (2, 2, "dense", "randn", "flat"), (256, 2, "dense", "offset", "flat"), (257, 2, "dense", "randn", "partial"),
    (65536, 2, "dense", "randn", "flat"), (65537, 2, "strided", "offset", "partial"),
    (1, 3, "dense", "randn", "partial"), (4, 3, "dense", "offset", "partial"), (255, 3, "strided", "randn", "partial"),
    (70001, 3, "strided", "offset", "partial"),
    (1, 4, "dense", "randn", "flat"), (3, 4, "dense", "offset", "flat"), (65537, 4, "dense", "offset", "flat"),
    (4, 4, "offset", "randn", "partial"), (257, 4, "strided", "randn", "partial"),
    (1, 64, "dense", "randn", "flat"), (255, 64, "dense", "offset", "flat"), (256, 64, "dense", "randn", "flat"),
    (257, 64, "dense", "offset", "flat"), (256, 64, "offset", "randn", "partial"), (257, 64, "strided", "randn", "partial"),
    (70001, 64, "dense", "randn", "flat"), (65537, 64, "strided", "offset", "partial"),
    (3, 128, "dense", "randn", "flat"), (4, 128, "offset", "offset", "partial"), (257, 128, "strided", "offset", "partial"),
    (1, 1024, "dense", "randn", "flat"), (3, 1024, "dense", "offset", "flat"), (256, 1024, "dense", "randn", "flat"),
    (257, 1024, "strided", "randn", "partial"),
    (1, 1025, "dense", "randn", "partial"), (4, 1025, "dense", "offset", "partial"), (257, 1025, "strided", "randn", "partial"),
    (3, 2048, "dense", "randn", "partial"), (255, 2048, "dense", "offset", "partial"), (4, 2048, "strided", "randn", "partial"),
]


@pytest.mark.parametrize("M,Cc,layout,data,route", COLSUM_CASES)
def test_colsum_against_float64(M, Cc, layout, data, route):
    L, dev = _lib()
    case = f"colsum M={M} C={Cc} {layout} {data} ({route})"
    gen = torch.Generator().manual_seed(1500 + M + 7 * Cc)
    x = torch.randn(M, Cc, generator=gen) + (100.0 if data == "offset" else 0.0)
    if layout == "offset":
        gx = _vec(M * Cc + 1, dev)                        # element 0 stays NaN; the operand starts 4 bytes behind it
        gx.view[0, 1:] = x.reshape(-1).to(dev)
        ptr, stride = gx.ptr + 4, Cc
    else:
        stride = Cc + 64 if layout == "strided" else Cc
        gx = Guarded(M, Cc, stride, dev, x)
        ptr = gx.ptr
    assert TS.colsum_route(M, Cc, stride, ptr) == route, f"{case}: the case does not reach the route it is there for"
    nblk = L.isi_colsum_num_partials(M)
    assert nblk == min((M + 255) // 256, 256)
    out, ws = _vec(Cc, dev), _vec(nblk * Cc, dev)
    _run(L, L.isi_colsum_f32(ptr, stride, out.ptr, ws.ptr, M, Cc, None))
    _assert_guards(case, out=out, workspace=ws, x=gx)
    _check(case, out.view.reshape(Cc), TS.colsum_spec(x), TS.colsum_f32(x), "out")


# ------------------------------------------------------------------------------------------------------------------ MSE
def _mse_case(n, forward=True, da=True, db=True):
    L, dev = _lib()
    case = f"mse n={n} fwd={int(forward)} da={int(da)} db={int(db)}"
    gen = torch.Generator().manual_seed(1600 + n % 9973)
    a, b, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen), 0.75
    ga, gb, gg = _vec(n, dev, a), _vec(n, dev, b), _vec(1, dev, torch.tensor([g]))
    ref, yard = TS.mse_spec(a, b, g), TS.mse_f32(a, b, g)
    if forward:
        np_ = L.isi_mse_loss_num_partials(n)
        assert np_ == max(1, min(1024, (n // 4 + 255) // 256))
        ws, out = _vec(np_, dev), _vec(1, dev)
        _run(L, L.isi_mse_loss_f32(ga.ptr, gb.ptr, n, ws.ptr, out.ptr, None))
        _assert_guards(case, workspace=ws, out=out, a=ga, b=gb)
        _check(case, out.view.reshape(1), ref[0], yard[0], "value")
    gda, gdb = _vec(n, dev) if da else None, _vec(n, dev) if db else None
    _run(L, L.isi_mse_loss_bwd_f32(ga.ptr, gb.ptr, gg.ptr, n, gda.ptr if da else None, gdb.ptr if db else None, None))
    _assert_guards(case, a=ga, b=gb, g=gg, **({"da": gda} if da else {}), **({"db": gdb} if db else {}))
    _unchanged(case, a=(ga, a), b=(gb, b))
    if da:
        _check(case, gda.view.reshape(n), ref[1], yard[1], "da")
    if db:
        _check(case, gdb.view.reshape(n), ref[2], yard[2], "db")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_mse_value_and_gradients_against_float64(n):
    _mse_case(n)


@pytest.mark.parametrize("n", [5, 1027])
@pytest.mark.parametrize("which", ["da", "db"])
def test_mse_backward_with_one_gradient(n, which):
    _mse_case(n, forward=False, da=which == "da", db=which == "db")


def test_mse_past_the_forward_cap():
    _mse_case(4 * 1024 * 256 + 1203)                      # 1024 blocks, second pass of the partial sums, tail of 3
    _release()


def test_mse_backward_past_the_grid_cap():
    _mse_case(4 * CAP + 1203, forward=False)
    _release()


# ---------------------------------------------------------------------------------------------------------- vq_finalize
# (K, n_part, N, draw of the counts).  K: 1, 7 inside one trip of the 256 threads, 256 / 512 whole trips, 1000 a ragged one,
# 2048 eight; n_part likewise 1, 256, 257; N: 1 and 37 leave most codes unused ("zeros": at most K / 16 + 1 codes are used at
# all), 2^20 is the largest count the bottom level sees at batch 64.
FINALIZE_CASES = [
    (1, 1, 1, "flat"), (1, 257, 2 ** 20, "flat"), (7, 1, 37, "flat"), (7, 256, 37, "zeros"), (256, 257, 65536, "flat"),
    (256, 256, 2 ** 20, "peaked"), (512, 257, 65536, "peaked"), (512, 1, 37, "zeros"), (1000, 256, 65536, "zeros"),
    (1000, 257, 2 ** 20, "flat"), (2048, 257, 2 ** 20, "flat"), (2048, 256, 65536, "peaked"), (2048, 1, 1, "zeros"),
]


@pytest.mark.parametrize("K,n_part,N,draw", FINALIZE_CASES)
def test_vq_finalize_against_float64(K, n_part, N, draw):
    L, dev = _lib()
    D = 64
    case = f"vq_finalize K={K} n_part={n_part} N={N} {draw}"
    gen = torch.Generator().manual_seed(1700 + K + n_part + N % 9973)
    if draw == "flat":
        idx = torch.randint(0, K, (N,), generator=gen)
    elif draw == "peaked":
        w = torch.exp(-torch.arange(K, dtype=torch.float32) * (8.0 / K))
        idx = torch.multinomial(w, N, replacement=True, generator=gen)
    else:
        used = torch.randperm(K, generator=gen)[:K // 16 + 1]
        idx = used[torch.randint(0, used.numel(), (N,), generator=gen)]
    counts = torch.bincount(idx, minlength=K).to(torch.int32)
    assert int(counts.sum()) == N
    sse = torch.rand(n_part, generator=gen) * (0.3 * N * D / n_part)
    gs, gc, out = _vec(n_part, dev, sse), IntGuarded(counts, dev, 2 ** 30), _vec(2, dev)
    _run(L, L.isi_vq_finalize_f32(gs.ptr, n_part, gc.ptr, K, N, D, out.ptr, None))
    _assert_guards(case, sse_part=gs, counts=gc, out2=out)
    ref, yard = TS.vq_finalize_spec(sse, counts, N, D), TS.vq_finalize_f32(sse, counts, N, D)
    got = out.view.reshape(2).cpu()
    _check(case, got[0:1], ref[0], yard[0], "diff")
    _check(case, got[1:2], ref[1], yard[1], "perplexity")


# -------------------------------------------------------------------------------------------------------- vq_ema_update
# (D, K): K = 1000 leaves 24 of the single workgroup's 1024 threads without a code, 1500 and 2048 give a thread two
@pytest.mark.parametrize("D,K", [(8, 32), (64, 512), (64, 1000), (16, 1500), (64, 2048)])
def test_vq_ema_update_against_float64(D, K):
    L, dev = _lib()
    case = f"vq_ema_update D={D} K={K}"
    decay, eps = 0.99, 1e-5
    state = TS.ema_state(D, K, torch.Generator().manual_seed(1800 + K))
    embed, cs, ea, counts, esum = state
    assert bool((counts == 0).any()) and bool((cs == 0).any())
    ge, ga, gsum = Guarded(D, K, K, dev, embed), Guarded(D, K, K, dev, ea), Guarded(D, K, K, dev, esum)
    gcs, gcnt = _vec(K, dev, cs), _vec(K, dev, counts)
    _run(L, L.isi_vq_ema_update_f32(ge.ptr, gcs.ptr, ga.ptr, gcnt.ptr, gsum.ptr, D, K, decay, eps, None))
    _assert_guards(case, embed=ge, cluster_size=gcs, embed_avg=ga, counts=gcnt, embed_sum=gsum)
    _unchanged(case, counts=(gcnt, counts), embed_sum=(gsum, esum))
    ref, yard = TS.ema_update_spec(*state, decay, eps), TS.ema_update_f32(*state, decay, eps)     # of the original contents
    _check(case, ge.view, ref[0], yard[0], "embed")
    _check(case, gcs.view.reshape(K), ref[1], yard[1], "cluster_size")
    _check(case, ga.view, ref[2], yard[2], "embed_avg")


# ----------------------------------------------------------------------------------------------------------- embed_code
@pytest.mark.parametrize("D,N,K", [(8, 1, 5), (16, 1, 37), (16, 5, 37), (32, 4097, 512), (64, 5, 2048), (64, 4097, 37), (8, 4097, 7)])
def test_embed_code_bit_for_bit(D, N, K):
    L, dev = _lib()
    case = f"embed_code D={D} N={N} K={K}"
    gen = torch.Generator().manual_seed(1900 + D + N + K)
    codes = torch.randn(K, D, generator=gen)
    idx = torch.randint(0, K, (N,), generator=gen)
    if N >= 5:
        idx[0], idx[1], idx[2], idx[3], idx[-1] = -1, K, 0, K - 1, 2 ** 40            # clamped: below, just above, far above
    else:
        idx[0] = K if D == 8 else -1
    gcodes, gidx, out = Guarded(K, D, D, dev, codes), IntGuarded(idx, dev, 2 ** 62), Guarded(N, D, D, dev)
    _run(L, L.isi_embed_code_f32(gidx.ptr, gcodes.ptr, out.ptr, N, D, K, None))
    _assert_guards(case, codes=gcodes, idx=gidx, out=out)
    _exact(case, out.view, TS.embed_code_spec(idx, codes, K), "out")


# ------------------------------------------------------------------------- pair round trip, relu_inplace, pad_channels4
def _pair_case(n):
    L, dev = _lib()
    case = f"pair encode/decode n={n}"
    gen = torch.Generator().manual_seed(2000 + n % 9973)
    x = torch.randn(n, generator=gen)
    x[:8] = torch.tensor([0.0, -0.0, 1000.0, -1000.0, 1e-6, 2.0 ** -20, -3.0, 0.1])
    gx, pairs, back = _vec(n, dev, x), _vec(n, dev), _vec(n, dev)     # (8 f16 hi + 8 f16 lo per 8 floats: n floats of pairs)
    _run(L, L.isi_pair_encode_f32(gx.ptr, pairs.ptr, n, None))
    _run(L, L.isi_pair_decode_f32(pairs.ptr, back.ptr, n, None))
    _assert_guards(case, x=gx, pairs=pairs, decoded=back)
    _unchanged(case, x=(gx, x))
    _exact(case, back.view.reshape(n), TS.pair_round_f16(x), "decoded")


@pytest.mark.parametrize("n", [8, 2056])
def test_pair_round_trip_bit_for_bit(n):
    _pair_case(n)


def test_pair_round_trip_past_the_grid_cap():
    _pair_case(8 * CAP + 2400)                            # one 67 MB pair buffer
    _release()


def test_relu_inplace_past_the_grid_cap():
    L, dev = _lib()
    n = 4096 * 256 + 77                                   # its launch is capped at 4096 blocks of scalars
    case = f"relu_inplace n={n}"
    x = torch.randn(n, generator=torch.Generator().manual_seed(2100))
    for at in (0, 1000, 4096 * 256 + 5):
        x[at:at + 6] = torch.tensor([NAN, -0.0, 0.0, float("inf"), float("-inf"), -2.0 ** -126])
    gx = _vec(n, dev, x)
    _run(L, L.isi_relu_inplace_f32(gx.ptr, n, None))
    _assert_guards(case, x=gx)
    got = gx.view.reshape(n).cpu()
    assert bool(torch.isnan(got[0])) and bool(torch.isnan(got[4096 * 256 + 5])), f"{case}: a NaN must stay NaN"
    _exact(case, got, TS.relu_inplace_spec(x), "x")
    _release()


def test_pad_channels4_past_the_grid_cap():
    from interactive_spectrogram_inpainting import _hip
    L, dev = _lib()
    B, Cc, H, W = 1, 2, 1025, 2048                        # 2 099 200 pixels against 2 097 152 threads
    case = f"pad_channels4 B={B} C={Cc} H={H} W={W}"
    base = torch.full((B, Cc + 1, H + 1, W + 3), NAN)
    base[:, 1:, :H, 1:W + 1] = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(2200))
    view = base.to(dev)[:, 1:, :H, 1:W + 1]               # a non-contiguous NCHW view with NaN all around it
    assert not view.is_contiguous()
    out = Guarded(B * H * W, 4, 4, dev)
    sv = _hip.src_nchw_view(view)
    _run(L, L.isi_pad_channels4_f32(C.byref(sv), out.ptr, B, H, W, None))
    _assert_guards(case, out=out)
    want = torch.nn.functional.pad(base[:, 1:, :H, 1:W + 1].permute(0, 2, 3, 1), (0, 4 - Cc)).reshape(B * H * W, 4)
    _exact(case, out.view, want, "out")
    _release()
