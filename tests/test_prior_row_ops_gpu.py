"""The prior's row-wise kernels against the float64 specifications of tests/tests_support.py, at every width and block
count where they take another path: layernorm_f32_kernel, layernorm_bwd_kernel<2|4|8> with layernorm_bwd_reduce_kernel,
label_smoothing_kernel and linear_rows_f32_kernel<1|4|8>.

Every comparison is `tests_support.compare_rows`: the kernel may be 8 times as far from the float64 spec as a float32 torch
evaluation of the same operation on the same data, in a per-row metric (a wrong row of small magnitude shows).  Every
output lies inside a larger buffer of NaN whose guard regions (before, behind, rows past M, columns between the width and
the stride) must keep their bits; every input lies in NaN too, so a read past a row's end poisons the result.
tests/test_prior_row_ops_host.py shows, without a GPU, what the comparison accepts and rejects.

A recording aid, not a check: with ISI_ROW_OPS_RECORD=<file> in the environment the measured error, yardstick and ratio of
every comparison are written there when the module ends, the worst ratio first (profiles/row_ops_checks.txt is such a run)."""
import ctypes as C
import os

import pytest
import torch

import tests_support as TS
from test_prior_gpu import _dev

pytestmark = pytest.mark.gpu

EPS = 1e-5
PAD = 64                       # floats of NaN before and behind every buffer (a multiple of 4: 16-byte alignment stays)
RECORD = []                    # (case, RowCheck) of every comparison of this process


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_ROW_OPS_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# kernel error, float32-torch yardstick (floored at 2^-23) and their ratio against the float64 spec, per comparison of\n"
                "# tests/test_prior_row_ops_gpu.py; metric and bound: tests_support.compare_rows (ratio <= 8).  Worst ratio first.\n")
        for case, c in sorted(RECORD, key=lambda r: -r[1].ratio):
            f.write(f"{c.ratio:8.3f}  err {c.err:.3e}  yardstick {c.yardstick:.3e}  {c.what}\n")


def _check(case, got, ref, yardstick, what, margin=TS.ROW_OPS_MARGIN):
    got = got.cpu()
    err, yard = TS.row_error(got, ref), max(TS.row_error(yardstick, ref), TS.ROW_OPS_FLOOR)
    print(f"{case} {what}: err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    RECORD.append((case, TS.compare_rows(got, ref, yardstick, f"{case} {what}", margin)))


class Guarded:
    """[rows, cols] view with row stride `stride` inside a flat NaN buffer: PAD floats in front, two more rows and PAD floats
    behind.  `src` fills the view (an input); without it the view stays NaN (an output, to be overwritten whole)."""

    def __init__(self, rows, cols, stride, dev, src=None, dtype=torch.float32):
        assert stride >= cols
        self.buf = torch.full((PAD + (rows + 2) * stride + PAD,), float("nan"), dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + rows * stride].view(rows, stride)[:, :cols]
        guard = torch.ones(self.buf.shape, dtype=torch.bool, device=dev)
        guard[PAD:PAD + rows * stride].view(rows, stride)[:, :cols] = False
        self.guard = guard
        if src is not None:
            self.view.copy_(src.reshape(rows, cols))
        self.bits = self.buf.view(torch.int32).clone()
        self.ptr = self.view.data_ptr()

    def intact(self):
        now = self.buf.view(torch.int32)
        return bool(torch.equal(now[self.guard], self.bits[self.guard]))


def _vec(n, dev, src=None):
    return Guarded(1, n, n, dev, src)


def _assert_guards(case, **bufs):
    for name, b in bufs.items():
        assert b.intact(), f"{case}: the kernel wrote outside {name}"


# ------------------------------------------------------------------------------------------------------------ LayerNorm
# (D, M, residual, dropout p, data).  D: every edge of lane + 64 i < D / 4 and of the backward's instantiations (<2>: D <= 512,
# <4>: <= 1024, <8>: <= 2048).  M: 1..9 inside one backward block and around the forward's four rows per workgroup;
# 392 / 393 rows = 49 / 50 blocks, where the reduce kernel's four-way loop first runs; 8193 rows = 1024 blocks of 9 rows,
# the last 113 of them empty.
LN_CASES = [
    (4, 1, False, 0.0, "randn"), (4, 9, True, 0.0, "offset"),
    (96, 3, True, 0.0, "randn"), (96, 392, False, 0.0, "const"),
    (252, 4, True, 0.0, "offset"), (252, 393, False, 0.0, "randn"),
    (256, 5, False, 0.0, "randn"), (256, 8, True, 0.0, "const"),
    (260, 8, True, 0.0, "randn"), (260, 392, False, 0.0, "offset"),
    (512, 9, True, 0.3, "randn"), (512, 393, False, 0.0, "offset"), (512, 8, False, 0.3, "offset"),
    (516, 1, True, 0.0, "const"), (516, 392, True, 0.3, "randn"), (516, 8193, True, 0.0, "randn"),
    (516, 8193, False, 0.0, "offset"),
    (768, 3, False, 0.0, "randn"), (768, 393, True, 0.0, "offset"),
    (1024, 4, True, 0.0, "randn"), (1024, 392, False, 0.0, "const"),
    (1028, 5, False, 0.3, "randn"), (1028, 393, True, 0.3, "offset"),
    (2044, 1, True, 0.0, "randn"), (2044, 9, False, 0.0, "offset"),
    (2048, 3, True, 0.3, "randn"), (2048, 393, True, 0.0, "randn"), (2048, 5, False, 0.3, "randn"),
    (2048, 4, False, 0.0, "const"),
    (64, 8193, False, 0.0, "offset"), (64, 8193, True, 0.3, "randn"),
]


def _ln_case_data(D, M, res, data, seed):
    g = torch.Generator().manual_seed(seed)
    x = TS.layernorm_data(data, M, D, g)
    r = torch.randn(M, D, generator=g) if res else None
    if res and data == "const":                          # the constant rows stay constant under the residual
        r[0], r[-1] = 1.0, 2.0
    if res and data == "offset":
        r *= 0.01                                        # (a residual of the data's own size would hide the 1e-3 rows)
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g)
    return x, r, gamma, beta, dy


def _ln_forward(L, x, r, gamma, beta, y, M, D, p, seed):
    rp = r.ptr if r is not None else None
    if p:
        return L.isi_layernorm_dropout_f32(x.ptr, rp, gamma.ptr, beta.ptr, y.ptr, M, D, EPS, p, seed, None)
    return L.isi_layernorm_f32(x.ptr, rp, gamma.ptr, beta.ptr, y.ptr, M, D, EPS, None)


def _ln_backward(L, x, r, gamma, dy, M, D, p, seed, dev):
    """One backward into fresh guarded buffers; the workspace has the size the C-ABI asks for and starts as NaN (a block
    that does not write its partial sums, an empty one included, poisons dgamma and dbeta)."""
    out = dict(dz=Guarded(M, D, D, dev), dgamma=_vec(D, dev), dbeta=_vec(D, dev),
               workspace=_vec(L.isi_layernorm_bwd_workspace_floats(M, D), dev))
    rp = r.ptr if r is not None else None
    if p:
        out["dx"] = Guarded(M, D, D, dev)
        rc = L.isi_layernorm_dropout_bwd_f32(x.ptr, rp, gamma.ptr, dy.ptr, out["dz"].ptr, out["dx"].ptr, out["dgamma"].ptr,
                                             out["dbeta"].ptr, out["workspace"].ptr, M, D, EPS, p, seed, None)
    else:
        rc = L.isi_layernorm_bwd_f32(x.ptr, rp, gamma.ptr, dy.ptr, out["dz"].ptr, out["dgamma"].ptr, out["dbeta"].ptr,
                                     out["workspace"].ptr, M, D, EPS, None)
    assert rc == 0, L.isi_last_error()
    return out


@pytest.mark.parametrize("D,M,res,p,data", LN_CASES)
def test_layernorm_forward_and_backward_against_float64(D, M, res, p, data):
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.priors import _ops, _train as PT
    L, dev = _hip.lib(), _dev()
    case = f"layernorm D={D} M={M} res={int(res)} p={p} {data}"
    seed_of_case = 1000 + 7 * D + M + int(res)
    x, r, gamma, beta, dy = _ln_case_data(D, M, res, data, seed_of_case)
    assert L.isi_layernorm_bwd_workspace_floats(M, D) == min(1024, (M + 7) // 8) * 2 * D
    torch.manual_seed(seed_of_case)
    seed = _ops.dropout_seed() if p else 0               # the seed LayerNormFn draws below, after the same manual_seed

    gx, gdy = Guarded(M, D, D, dev, x), Guarded(M, D, D, dev, dy)
    gr = Guarded(M, D, D, dev, r) if res else None
    gg, gb = _vec(D, dev, gamma), _vec(D, dev, beta)
    gy = Guarded(M, D, D, dev)
    assert _ln_forward(L, gx, gr, gg, gb, gy, M, D, p, seed) == 0, L.isi_last_error()
    b1 = _ln_backward(L, gx, gr, gg, gdy, M, D, p, seed, dev)
    b2 = _ln_backward(L, gx, gr, gg, gdy, M, D, p, seed, dev)
    torch.cuda.synchronize()
    _assert_guards(case, y=gy, x=gx, dy=gdy, gamma=gg, beta=gb, **b1)
    for name in ("dz", "dgamma", "dbeta"):               # fixed-order sums: the same bits on equal inputs
        assert torch.equal(b1[name].view.view(torch.int32), b2[name].view.view(torch.int32)), f"{case}: {name} differs between two calls"

    keep = None
    if p:
        keep = (b1["dx"].view != 0).cpu()                # (a kept element's gradient is exactly 0 with probability 0)
        if M * D >= 100000:
            assert abs(1.0 - keep.double().mean().item() - p) < 0.01
    y_ref = TS.layernorm_spec(x, r, gamma, beta, EPS, keep, p)
    _check(case, gy.view, y_ref, TS.layernorm_f32(x, r, gamma, beta, EPS, keep, p)[0], "y")
    refs = TS.layernorm_bwd_spec(x, r, gamma, dy, EPS, keep, p)
    yards = TS.layernorm_bwd_f32(x, r, gamma, dy, EPS, keep, p)
    for i, name in enumerate(("dz", "dx", "dgamma", "dbeta")):
        if name == "dx" and not p:
            continue
        got = b1[name].view.reshape(refs[i].shape)
        _check(case, got, refs[i], yards[i], name)
    if data == "const":
        # variance 0.  The constants (layernorm_data; 4.75 and 1.75 with the residual) have five significant bits, so the sum
        # of up to 2048 of them is exact in fp32 in any order: mean = the constant, xhat = 0 and y = beta, exactly
        assert torch.equal(gy.view[[0, M - 1]].cpu(), beta.expand(2, D)), f"{case}: a constant row must give beta"

    # the Python entries: the same launches behind LayerNormFn, bit for bit
    xd, gd, bd = (t.to(dev).requires_grad_(True) for t in (x, gamma, beta))
    rd = r.to(dev).requires_grad_(True) if res else None
    torch.manual_seed(seed_of_case)
    y = PT.LayerNormFn.apply(xd, rd, gd, bd, EPS, p)
    y.backward(dy.to(dev))
    assert torch.equal(y.detach(), gy.view), f"{case}: LayerNormFn's forward"
    assert torch.equal(xd.grad, (b1["dx"] if p else b1["dz"]).view), f"{case}: LayerNormFn's dx"
    if res:
        assert torch.equal(rd.grad, b1["dz"].view), f"{case}: LayerNormFn's dres"
    assert torch.equal(gd.grad, b1["dgamma"].view.reshape(D)) and torch.equal(bd.grad, b1["dbeta"].view.reshape(D)), case
    if not p:
        assert torch.equal(_ops.layernorm(xd.detach(), gd.detach(), bd.detach(), EPS, residual=rd.detach() if res else None),
                           gy.view), f"{case}: _ops.layernorm"


# ------------------------------------------------------------------------------------------------------ label smoothing
# (K, M, num_classes - K, smoothing, logits, with gradient).  K: one class per lane and less (2, 17, 63, 64), the second
# trip of the lane loops (65), the production sizes 512 and 513 (the top prior's mask token: num_classes = K - 1), 1024.
# M: 1, 3, 5 leave waves of the last workgroup without a row; 4100 = 1025 workgroups.
LS_CASES = [
    (2, 1, 0, 0.1, "randn", True), (2, 5, 0, 0.0, "const", True),
    (17, 3, -1, 0.1, "randn", True), (17, 4, 0, 0.0, "peaked", False),
    (63, 4, 0, 0.1, "shifted", True), (63, 5, -1, 0.0, "randn", True),
    (64, 1, -1, 0.1, "peaked", True), (64, 4100, 0, 0.1, "randn", True),
    (65, 3, 0, 0.1, "const", True), (65, 5, -1, 0.0, "shifted", False),
    (512, 4100, 0, 0.1, "peaked", True), (512, 3, -1, 0.1, "randn", False),
    (513, 4100, -1, 0.1, "shifted", True), (513, 1, 0, 0.0, "peaked", True), (513, 4, -1, 0.1, "peaked", True),
    (1024, 4, -1, 0.1, "const", True), (1024, 5, 0, 0.1, "peaked", True), (1024, 4100, 0, 0.0, "randn", True),
]


@pytest.mark.parametrize("idx", range(len(LS_CASES)), ids=[f"K{c[0]}-M{c[1]}-nc{c[2]}-s{c[3]}-{c[4]}-g{int(c[5])}" for c in LS_CASES])
def test_label_smoothing_against_float64(idx):
    """Regression of the fault these tests found: for K != num_classes with smoothing > 0 (K = 17 / 64 / 513 / 1024 with
    num_classes = K - 1 here) the kernel wrote (softmax - true_dist) * grad_scale, which is the gradient of its own row
    loss only where true_dist sums to 1; at K = 17, smoothing 0.1 the softmax term was off by 0.67 %."""
    from interactive_spectrogram_inpainting import _hip
    K, M, dnc, smoothing, kind, with_grad = LS_CASES[idx]
    L, dev = _hip.lib(), _dev()
    nc = K + dnc
    case = f"label_smoothing K={K} M={M} num_classes={nc} s={smoothing} {kind} grad={int(with_grad)}"
    g = torch.Generator().manual_seed(2000 + idx)
    logits = torch.randn(M, K, generator=g)
    if kind == "peaked":
        logits *= 30.0                                   # most exp() underflow
    elif kind == "shifted":
        logits += 1000.0                                 # the shift must cancel
    elif kind == "const":
        logits = (torch.randn(M, 1, generator=g) * 5.0).expand(M, K).contiguous()
    target = torch.randint(0, K, (M,), generator=g)
    special = [0, K - 1, 64 + (K - 65) // 2 if K > 64 else K // 2]   # first, last, one at or above 64 where K allows
    for row in range(min(M, 3)):
        target[row] = special[(row + idx) % 3]
    grad_scale = 0.75 / M

    gl = Guarded(M, K, K, dev, logits)
    tgt = target.to(dev)
    loss = _vec(M, dev)
    dl = Guarded(M, K, K, dev) if with_grad else None
    rc = L.isi_label_smoothing_loss_f32(gl.ptr, tgt.data_ptr(), loss.ptr, dl.ptr if with_grad else None, M, K, nc,
                                        smoothing, grad_scale, None)
    assert rc == 0, L.isi_last_error()
    torch.cuda.synchronize()
    _assert_guards(case, logits=gl, row_loss=loss, **({"dlogits": dl} if with_grad else {}))
    ref_loss, ref_grad = TS.label_smoothing_spec(logits, target, nc, smoothing, grad_scale)
    yard_loss, yard_grad = TS.label_smoothing_f32(logits, target, nc, smoothing, grad_scale)
    _check(case, loss.view.reshape(M), ref_loss, yard_loss, "row_loss")
    if not with_grad:
        return
    _check(case, dl.view, ref_grad, yard_grad, "dlogits")
    # Row sums.  In exact arithmetic a row of the gradient sums to (td_sum - sum_k true_dist) * grad_scale = 0: the softmax
    # sums to 1 and weighs td_sum = sum_k true_dist = on + (K - 1) off.  (For K == num_classes td_sum = 1 and this is the row
    # sum (1 - on - (K - 1) off) * grad_scale of softmax - true_dist.)  Rounding, in units of u = 2^-24 of grad_scale: the
    # probabilities are the kernel's own exp terms over their fp32 sum, so they sum to 1 within the error of that sum
    # (K / 64 serial adds per lane + 6 butterfly levels, all terms positive) plus 1 for the reciprocal and 1 for each
    # product; the K subtractions of true_dist round by at most u max(p, true_dist) each, 2 in sum; on, off and td_sum are
    # fp32 roundings of sums that are 1, 3 together; the product with grad_scale 1.  K / 64 + 14, taken as K / 64 + 16 at
    # u = 2^-23 for the terms bounded to first order.
    sums = dl.view.cpu().double().sum(dim=1)
    bound = grad_scale * 2.0 ** -23 * (K / 64 + 16)
    print(f"{case} row sums: max |sum| {float(sums.abs().max()):.3e} bound {bound:.3e}")
    assert float(sums.abs().max()) <= bound, f"{case}: a gradient row sums to {float(sums.abs().max()):.3e}, bound {bound:.3e}"


def test_label_smoothing_python_entry_matches_the_oracle_gradient():
    """LabelSmoothingLoss -> label_smoothing_loss -> LabelSmoothingFn at the top prior's shape (513 logits, 512 classes):
    the loss and its autograd gradient against float64 autograd of oracle/prior_oracle.py."""
    from oracle import prior_oracle as P
    from interactive_spectrogram_inpainting.utils.losses.prediction import LabelSmoothingLoss
    dev = _dev()
    g = torch.Generator().manual_seed(2100)
    pred = 3.0 * torch.randn(3, 513, 7, generator=g)
    target = torch.randint(0, 513, (3, 7), generator=g)
    pd = pred.to(dev).requires_grad_(True)
    loss = LabelSmoothingLoss(512, 0.1, dim=1)(pd, target.to(dev))
    (loss * 0.75).backward()
    p64 = pred.double().requires_grad_(True)
    ref = P.label_smoothing_loss(p64, target, 512, 0.1, dim=1)
    (ref * 0.75).backward()
    p32 = pred.clone().requires_grad_(True)
    (P.label_smoothing_loss(p32, target, 512, 0.1, dim=1) * 0.75).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 8 * 2.0 ** -23 * abs(float(ref.detach()))
    rows = lambda t: t.detach().cpu().movedim(1, -1).reshape(-1, 513)
    _check("label_smoothing LabelSmoothingLoss 513/512", rows(pd.grad), rows(p64.grad), rows(p32.grad), "dpred")


# ---------------------------------------------------------------------------------------------------------- linear_rows
# (M, K, N, x_stride - K, res_stride - N, out_stride - N, bias, residual, relu).  M = 1: <1>; 2, 4: <4>; 5, 8: <8>.
LR_CASES = [
    (1, 4, 1, 0, 0, 0, True, False, False), (1, 256, 513, 8, 0, 3, False, True, True),
    (1, 2048, 5, 0, 3, 0, True, True, False), (1, 252, 4, 0, 0, 3, False, False, False),
    (2, 252, 3, 8, 3, 3, True, True, True), (2, 260, 50, 0, 0, 0, False, False, False),
    (2, 2048, 4, 8, 0, 3, True, False, True), (2, 4, 5, 8, 3, 0, False, True, True),
    (4, 4, 513, 0, 3, 3, True, True, False), (4, 256, 1, 8, 0, 0, False, False, False),
    (4, 260, 5, 8, 3, 0, True, True, True), (4, 2048, 3, 0, 0, 3, False, True, False),
    (5, 252, 50, 0, 0, 3, True, False, False), (5, 2048, 513, 8, 3, 3, False, True, False),
    (5, 4, 3, 8, 0, 0, True, False, True), (5, 256, 5, 0, 0, 0, True, False, False),
    (8, 256, 4, 0, 3, 3, True, True, False), (8, 260, 1, 8, 3, 3, False, True, False),
    (8, 252, 513, 0, 0, 0, True, False, True), (8, 2048, 50, 8, 3, 3, True, True, True),
]


@pytest.mark.parametrize("M,K,N,dxs,drs,dos,bias,res,relu", LR_CASES)
def test_linear_rows_against_float64(M, K, N, dxs, drs, dos, bias, res, relu):
    from interactive_spectrogram_inpainting import _hip
    L, dev = _hip.lib(), _dev()
    case = f"linear_rows M={M} K={K} N={N} strides+{dxs}/{drs}/{dos} bias={int(bias)} res={int(res)} relu={int(relu)}"
    g = torch.Generator().manual_seed(3000 + 31 * M + 7 * K + N)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(M, N, generator=g) if res else None
    gx, gw = Guarded(M, K, K + dxs, dev, x), Guarded(N, K, K, dev, W)
    gb = _vec(N, dev, b) if bias else None
    gr = Guarded(M, N, N + drs, dev, r) if res else None
    out = Guarded(M, N, N + dos, dev)
    rc = L.isi_linear_rows_f32(gx.ptr, K + dxs, gw.ptr, gb.ptr if bias else None, gr.ptr if res else None,
                               N + drs if res else 0, out.ptr, N + dos, M, N, K, int(relu), None)
    assert rc == 0, L.isi_last_error()
    torch.cuda.synchronize()
    _assert_guards(case, out=out, x=gx, W=gw)
    _check(case, out.view, TS.linear_rows_spec(x, W, b, r, relu), TS.linear_rows_f32(x, W, b, r, relu), "out")
