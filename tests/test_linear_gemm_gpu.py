"""The linear layers' GEMM (csrc/gemm_split_f32.hip, through isi_linear_f32) against the float64 specification of
tests/tests_support.py on every tile route: 128x64, 128x128, 256x128 and 256x256, each in both product modes
(ISI_CONV_BF16X3, ISI_CONV_F16X3) and with both weight forms (the fp32 weight, and the pair copy staged by plain copies),
with and without tail rows, and with every tail of the epilogue -- bias, residual, ReLU, gate with its scale, hash-masked
dropout.  Every case first asserts the route: isi_linear_route == tests_support.linear_route == the tile the case is for.

Every launch goes through ctypes with four independent row strides: x at ldx = K + 32 from column 16, the residual at
ldr = N + 4, the gate at ldg = N + 1, the output at ldo = N + 3 (no multiple of 4: the dropout mask is indexed by
m ldo + n).  x, residual, gate and output are views inside NaN buffers whose guards (in front, behind, between the row
width and the row stride) must keep their bits; the inputs must be unchanged.  The pair-copy launch must give the
fp32-weight launch's bits.  Each result is held by `tests_support.linear_hold`: the spec's zeros are zeros (dropped by the
mask, gated off, rectified), what it keeps is not, and tile rows and tail rows go through `compare_rows` (margin 8, floor
2^-23) as blocks of their own -- the tile rows against the worse of the float32 evaluation and the mode's three-term model,
the tail rows (plain fp32 dot products) against the float32 evaluation alone.  tests/test_linear_gemm_host.py shows,
without a GPU, what that comparison rejects.

The two wide shapes (N = 512, M = 64 and 128 rows per compute unit: 8.4 M and 16.8 M outputs on 256 CUs) are the smallest
that reach the 256-row tiles, which want a whole round of the chip; their references are torch's float64 / float32
matmuls on the device, everything else follows the CPU convention.

A recording aid, not a check: with ISI_LINEAR_GEMM_RECORD=<file> in the environment every comparison's error, yardstick
and ratio are written there when the module ends, the worst ratio first (profiles/linear_gemm_checks.txt is such a run on
an MI355X: the worst ratio there is 1.06, 128x64 tiles at M = 256, N = 40 in the f16 mode; per route 1.06 (128x64),
1.01 (128x128), 1.02 (256x128) and 1.01 (256x256) in the tile rows -- the bf16 mode sits at 1.0, its error being the three-term
truncation the yardstick models -- and 0.66 in the tail rows)."""
import contextlib
import ctypes as C
import functools
import os

import pytest
import torch

import tests_support as TS
from test_prior_gpu import _dev
from test_prior_row_ops_gpu import PAD, Guarded, _assert_guards

pytestmark = pytest.mark.gpu

RECORD = []                    # RowCheck of every comparison of this process
MODES = {"bf16": 2, "f16": 8}                             # ISI_CONV_BF16X3, ISI_CONV_F16X3
PAIR = {"bf16": 256, "f16": 16}                           # ISI_CONV_W16_BF16, ISI_CONV_W16
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_LINEAR_GEMM_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# kernel error, yardstick (floored at 2^-23) and their ratio against the float64 spec, per comparison of\n"
                f"# tests/test_linear_gemm_gpu.py; metric and bound: tests_support.compare_rows (ratio <= {TS.ROW_OPS_MARGIN:g}).  Worst ratio first.\n")
        for c in sorted(RECORD, key=lambda r: -r.ratio):
            f.write(f"{c.ratio:8.3f}  err {c.err:.3e}  yardstick {c.yardstick:.3e}  {c.what}\n")


class GuardedAt(Guarded):
    """Guarded with the view starting at column `col0` of the rows (x: column 16 of rows of K + 32)."""

    def __init__(self, rows, cols, stride, col0, dev, src=None):
        assert col0 + cols <= stride
        self.buf = torch.full((PAD + (rows + 2) * stride + PAD,), NAN, dtype=torch.float32, device=dev)
        self.view = self.buf[PAD:PAD + rows * stride].view(rows, stride)[:, col0:col0 + cols]
        guard = torch.ones(self.buf.shape, dtype=torch.bool, device=dev)
        guard[PAD:PAD + rows * stride].view(rows, stride)[:, col0:col0 + cols] = False
        self.guard = guard
        if src is not None:
            self.view.copy_(src.reshape(rows, cols))
        self.bits = self.buf.view(torch.int32).clone()
        self.ptr = self.view.data_ptr()


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _lib():
    from interactive_spectrogram_inpainting import _hip
    return _hip, _hip.lib(), _dev()


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@contextlib.contextmanager
def _knobs(_hip, knobs):
    with contextlib.ExitStack() as st:
        for name, value in knobs:
            st.enter_context(_hip.knob(name, value))
        yield


def _seed_base():
    """The device-resident term the library adds to every fused dropout's seed, if an earlier test of the process left one."""
    from interactive_spectrogram_inpainting.priors import _ops
    return int(_ops._SEED_BASE.item()) if _ops._SEED_BASE is not None else 0


class Operands:
    """A case's operands on the device: x, residual and gate inside NaN buffers, the weight in its three forms."""

    def __init__(self, c, refs, dev):
        from interactive_spectrogram_inpainting.priors import _ops
        M, N, K = c.M, c.N, c.K
        self.c, self.dev, self.refs = c, dev, refs
        self.x = GuardedAt(M, K, K + 32, 16, dev, refs.x)
        self.res = Guarded(M, N, N + 4, dev, refs.res)
        self.gate = Guarded(M, N, N + 1, dev, refs.gate)
        self.bias = refs.bias.to(dev)
        self.W = refs.W.to(dev).contiguous()
        self.w32 = _ops.pack_linear_weight(self.W, range_check="now")
        self.w16 = {"f16": _ops.pack_linear_weight(self.W, range_check="now", with_f16=True)}
        assert self.w16["f16"].isi_w16
        # the bf16 pair copy as the input-gradient GEMMs get it: pack_linear_weight_t of the transposed weight (it has the
        # pair copy for multiples of 32 only; a ragged N runs the bf16 mode with the fp32 weight alone)
        self.Wt = self.W.t().contiguous()
        wt = _ops.pack_linear_weight_t(self.Wt)
        assert bool(getattr(wt, "isi_w16_bf16", False)) == (N % 32 == 0)
        if N % 32 == 0:
            assert _bits_equal(wt[:N * K].view(N, K), self.W), "the fp32 part of the transposed pack is the weight"
            self.w16["bf16"] = wt

    def launch(self, L, mode, pair, e, seed):
        """One isi_linear_f32 into a fresh NaN output; returns the Guarded output."""
        from interactive_spectrogram_inpainting import _hip
        c = self.c
        bias, res, relu, gate, gate_scale, keep, p = e
        out = Guarded(c.M, c.N, c.N + 3, self.dev)
        a = _hip.isi_linear_args()
        a.x, a.ldx = self.x.ptr, c.K + 32
        a.packed_w = (self.w16[mode] if pair else self.w32).data_ptr()
        a.bias = self.bias.data_ptr() if bias is not None else None
        if res is not None:
            a.residual, a.ldr = self.res.ptr, c.N + 4
        if gate is not None:
            a.gate, a.ldg, a.gate_scale = self.gate.ptr, c.N + 1, gate_scale
        a.out, a.ldo, a.M, a.N, a.K = out.ptr, c.N + 3, c.M, c.N, c.K
        a.flags = int(relu) | MODES[mode] | (PAIR[mode] if pair else 0)
        a.drop_p, a.drop_seed = float(p), int(seed)
        rc = L.isi_linear_f32(C.byref(a), None)
        assert rc == 0, L.isi_last_error()
        torch.cuda.synchronize()
        return out

    def untouched(self, what, out):
        _assert_guards(what, x=self.x, residual=self.res, gate=self.gate, out=out)
        for name, g, src in (("x", self.x, self.refs.x), ("residual", self.res, self.refs.res), ("gate", self.gate, self.refs.gate)):
            assert _bits_equal(g.view, src.to(self.dev)), f"{what}: the kernel changed its input {name}"


def _hold(what, got, exp):
    try:
        checks = TS.linear_hold(got, exp, what)
    finally:    # (the figures are printed whether the comparison passes or not)
        M = exp.spec.shape[0]
        for name, rows in (("tile rows", slice(0, M - exp.tail)), ("tail rows", slice(M - exp.tail, M))):
            if rows.start != rows.stop:
                err = TS.row_error(got[rows], exp.spec[rows])
                yard = max(TS.row_error(exp.yard[rows], exp.spec[rows]), TS.ROW_OPS_FLOOR)
                print(f"{what} {name}: err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    RECORD.extend(checks)


def _run_case(c, epilogues, ref_device):
    _hip, L, dev = _lib()
    cus = _cus(dev)
    kn = dict(c.knobs)
    want = c.tile | c.tail << 8
    M, N, K = c.M, c.N, c.K
    refs = TS.linear_case_refs(M, N, K) if ref_device == "cpu" else _wide_refs(M, N, K, str(dev))
    ops = Operands(c, refs, dev)
    ldo = N + 3
    seeds = [(s + _seed_base()) & (2 ** 64 - 1) for s in TS.LINEAR_SEEDS]          # what the kernel hashes
    keeps = [TS.dropout_keep_mask(s, M, N, ldo, TS.LINEAR_DROP_P).to(refs.prod64.device) for s in seeds]
    assert not torch.equal(keeps[0], keeps[1])
    ran_pair = set()
    with _knobs(_hip, c.knobs):
        for mode, flag in MODES.items():
            for fl in (flag, flag | PAIR[mode]):
                route = L.isi_linear_route(M, N, K, fl)
                assert route == TS.linear_route(M, N, K, cus, kn.get("ISI_GEMM_NARROW_BELOW", 0), kn.get("ISI_GEMM_NO_WIDE", 0))
                assert route == want, f"the case is for {TS.LINEAR_TILES[c.tile]} with {c.tail} tail rows, the library routes {route:#x}"
            for which in epilogues:
                what = f"{TS.LINEAR_TILES[c.tile]} {M}x{N}x{K} {mode} {which}"
                e = TS.linear_epilogue_args(which, M, N, ldo, refs.bias, refs.res, refs.gate, keep=keeps[0])
                exp = TS.linear_expect(refs.prod64, refs.prod32, refs.model[mode], c.tail, *e)
                out = ops.launch(L, mode, False, e, TS.LINEAR_SEEDS[0])
                ops.untouched(what, out)
                _hold(what, out.view, exp)
                if mode in ops.w16:
                    out16 = ops.launch(L, mode, True, e, TS.LINEAR_SEEDS[0])
                    ops.untouched(what + " pair copy", out16)
                    assert _bits_equal(out16.view, out.view), f"{what}: the pair-copy launch differs from the fp32-weight launch"
                    ran_pair.add(mode)
                if e[5] is not None:    # another seed: another mask, held like the first; the same seed: the same bits
                    e2 = e[:5] + (keeps[1], e[6])
                    out2 = ops.launch(L, mode, False, e2, TS.LINEAR_SEEDS[1])
                    assert not torch.equal(out2.view == 0, out.view == 0), f"{what}: two seeds drew one mask"
                    _hold(what + " second seed", out2.view, TS.linear_expect(refs.prod64, refs.prod32, refs.model[mode], c.tail, *e2))
                    assert _bits_equal(ops.launch(L, mode, False, e, TS.LINEAR_SEEDS[0]).view, out.view), f"{what}: not reproducible"
                if c.knobs and c.knobs[0][0] == "ISI_GEMM_NO_WIDE":
                    # the same rows on the tile the default knobs select: the same bits
                    with _hip.knob("ISI_GEMM_NO_WIDE", 0):
                        assert L.isi_linear_route(M, N, K, flag) & 255 == 4
                        wide = ops.launch(L, mode, False, e, TS.LINEAR_SEEDS[0])
                    assert _bits_equal(wide.view, out.view), f"{what}: differs from the 256x256 tiles' result"
    assert ran_pair == ({"bf16", "f16"} if N % 32 == 0 else {"f16"})


@functools.lru_cache(maxsize=2)
def _wide_refs(M, N, K, dev):
    return TS.linear_refs(M, N, K, dev)


def _case_id(c):
    return f"{TS.LINEAR_TILES[c.tile]}-{c.M}x{c.N}x{c.K}" + "".join(f"-{k[4:].lower()}{v}" for k, v in c.knobs)


SMALL = TS.linear_cases(256)[0]                            # (the small shapes do not depend on the CU count)
N_WIDE = len(TS.linear_cases(256)[1])


@pytest.mark.parametrize("c", SMALL, ids=_case_id)
def test_linear_gemm_small_shapes(c):
    _run_case(c, TS.LINEAR_EPILOGUES, "cpu")


@pytest.mark.parametrize("i", range(N_WIDE))
def test_linear_gemm_wide_tiles(i):
    """The 256-row tiles: shapes written in terms of the device's CU count (tests_support.linear_cases)."""
    dev = _dev()
    c = TS.linear_cases(_cus(dev))[1][i]
    print(_case_id(c))
    _run_case(c, (TS.LINEAR_EPILOGUES[0], TS.LINEAR_EPILOGUES[-1]), "device")


def test_every_route_is_covered():
    """All four tiles x two modes x two weight forms are among the cases above (each asserts its route), each tile with and
    without tail rows where the kernel has them."""
    small, wide = TS.linear_cases(_cus(_dev()))
    for tile in (1, 2, 3, 4):
        cs = [c for c in small + wide if c.tile == tile]
        assert any(c.tail for c in cs) and any(not c.tail for c in cs), tile
        assert any(c.N % 32 == 0 for c in cs), "a case that runs the bf16 pair copy"
        assert {c.K // 32 % 2 for c in cs} == {0, 1}, "both parities of the two-stage ring"


def test_nan_stays_in_its_row():
    """A NaN in one element of x, in a tile row and in a tail row, with the ReLU: exactly those output rows are NaN in all N
    columns, every other row is finite and within the bounds."""
    _hip, L, dev = _lib()
    c = next(c for c in SMALL if (c.M, c.N, c.K) == (1030, 192, 128))
    assert L.isi_linear_route(c.M, c.N, c.K, 8) == 1 | 6 << 8
    refs = TS.linear_case_refs(c.M, c.N, c.K)
    rows = [5, c.M - 3]                                   # a tile row; a tail row (the last 6 rows)
    x = refs.x.clone()
    x[rows[0], 77] = NAN
    x[rows[1], 3] = NAN
    ops = Operands(c, refs._replace(x=x), dev)
    e = TS.linear_epilogue_args("bias+res+relu", c.M, c.N, c.N + 3, refs.bias, refs.res, refs.gate)
    for mode in MODES:
        for pair in (False, True):
            what = f"NaN rows {mode} pair={pair}"
            out = ops.launch(L, mode, pair, e, 0)
            _assert_guards(what, x=ops.x, residual=ops.res, out=out)
            got = out.view.cpu()
            assert bool(torch.isnan(got[rows]).all()), f"{what}: a NaN of x was rectified away"
            exp = TS.linear_expect(refs.prod64, refs.prod32, refs.model[mode], c.tail, *e)
            got[rows] = exp.spec[rows].float()
            _hold(what, got, exp)
