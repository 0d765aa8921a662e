"""CPU-side half of the row-kernel checks (tests/test_prior_row_ops_gpu.py holds the kernels themselves): the closed-form
float64 specifications of tests/tests_support.py equal float64 autograd; `compare_rows` accepts a float32 torch evaluation
of every operation and rejects the faults the GPU tests exist for, each applied to that float32 evaluation; the C-ABI
refuses, before any launch, the shapes the kernels are not laid out for."""
import pytest
import torch
import torch.nn.functional as F

import tests_support as TS

EPS = 1e-5
# (M, D or K, with residual / num_classes = K - 1, dropout p / smoothing)
SMALL = [(3, 8, True, 0.0), (5, 36, False, 0.3), (7, 260, True, 0.3)]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _ln_inputs(M, D, res, seed, kind="randn"):
    g = torch.Generator().manual_seed(seed)
    x = TS.layernorm_data(kind, M, D, g)
    r = torch.randn(M, D, generator=g) if res else None
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g)
    return g, x, r, gamma, beta, dy


@pytest.mark.parametrize("M,D,res,p", SMALL)
def test_layernorm_specs_equal_float64_autograd(M, D, res, p):
    g, x, r, gamma, beta, dy = _ln_inputs(M, D, res, 100 + D)
    keep = (torch.rand(M, D, generator=g) >= p) if p else None
    xd = x.double().requires_grad_(True)
    rd = r.double().requires_grad_(True) if res else None
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = xd * keep.double() / (1.0 - p) if p else xd
    y = F.layer_norm(z + rd if res else z, (D,), gd, bd, EPS)
    (y * dy.double()).sum().backward()
    assert _rel(TS.layernorm_spec(x, r, gamma, beta, EPS, keep, p), y.detach()) <= 1e-12
    dz, dx, dgamma, dbeta = TS.layernorm_bwd_spec(x, r, gamma, dy, EPS, keep, p)
    assert _rel(dx, xd.grad) <= 1e-12 and _rel(dgamma, gd.grad) <= 1e-12 and _rel(dbeta, bd.grad) <= 1e-12
    if res:
        assert _rel(dz, rd.grad) <= 1e-12
    if not p:
        assert dx is dz


@pytest.mark.parametrize("M,K,fewer,smoothing", [(3, 2, False, 0.1), (5, 17, True, 0.0), (7, 70, True, 0.1)])
def test_label_smoothing_spec_equals_float64_autograd_of_the_oracle(M, K, fewer, smoothing):
    from oracle import prior_oracle as P
    g = torch.Generator().manual_seed(200 + K)
    logits = 3.0 * torch.randn(M, K, generator=g)
    target = torch.randint(0, K, (M,), generator=g)
    nc = K - 1 if fewer else K
    ld = logits.double().requires_grad_(True)
    loss = P.label_smoothing_loss(ld, target, nc, smoothing, dim=1)
    (loss * 0.75).backward()
    row_loss, dlogits = TS.label_smoothing_spec(logits, target, nc, smoothing, 0.75 / M)
    assert abs(float(row_loss.mean() - loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert _rel(dlogits, ld.grad) <= 1e-12
    # the row losses one by one: the oracle on a single row
    for m in range(M):
        one = P.label_smoothing_loss(logits[m:m + 1].double(), target[m:m + 1], nc, smoothing, dim=1)
        assert abs(float(row_loss[m] - one)) <= 1e-12 * abs(float(one))


@pytest.mark.parametrize("M,K,N,bias,res,relu", [(1, 4, 1, True, False, False), (5, 36, 7, False, True, True),
                                                  (8, 260, 50, True, True, False)])
def test_linear_rows_spec_equals_float64_torch(M, K, N, bias, res, relu):
    g = torch.Generator().manual_seed(300 + K)
    x, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(M, N, generator=g) if res else None
    y = F.linear(x.double(), W.double(), b.double() if bias else None)
    if res:
        y = y + r.double()
    if relu:
        y = F.relu(y)
    assert _rel(TS.linear_rows_spec(x, W, b, r, relu), y) <= 1e-12


@pytest.mark.parametrize("kind", ["randn", "offset"])
def test_compare_rows_accepts_float32_torch(kind):
    """torch's own float32 kernels (layer_norm, log_softmax, linear and their autograd) pass against the plain float32
    evaluation as yardstick: the margin leaves room for another order of the same roundings.  (Not on the constant rows
    of layernorm_data: their constants make every plain sum exact, so an implementation that sums is held to xhat = 0
    exactly, and torch's layer_norm, which updates a running mean, is not one.)"""
    M, D = 37, 260
    g, x, r, gamma, beta, dy = _ln_inputs(M, D, True, 400, kind)
    xg, rg, gg, bg = (t.clone().requires_grad_(True) for t in (x, r, gamma, beta))
    y = F.layer_norm(xg + rg, (D,), gg, bg, EPS)
    (y * dy).sum().backward()
    ys = TS.layernorm_f32(x, r, gamma, beta, EPS)[0]
    TS.compare_rows(y.detach(), TS.layernorm_spec(x, r, gamma, beta, EPS), ys, "y")
    spec, yard = TS.layernorm_bwd_spec(x, r, gamma, dy, EPS), TS.layernorm_bwd_f32(x, r, gamma, dy, EPS)
    for got, s, f, name in zip((xg.grad, rg.grad, gg.grad, bg.grad), spec, yard, ("dz", "dx", "dgamma", "dbeta")):
        c = TS.compare_rows(got, s, f, name)
        assert c.what == name and c.ratio == c.err / c.yardstick and c.yardstick >= TS.ROW_OPS_FLOOR
    if kind != "randn":
        return
    K = 70
    logits = 30.0 * torch.randn(M, K, generator=g)
    target = torch.randint(0, K, (M,), generator=g)
    lg = logits.clone().requires_grad_(True)
    logp = F.log_softmax(lg, dim=1)
    true = torch.full((M, K), 0.1 / (K - 2))
    true[torch.arange(M), target] = 0.9
    rows = -(true * logp).sum(dim=1)
    (rows.sum() * 0.5).backward()
    spec, yard = TS.label_smoothing_spec(logits, target, K - 1, 0.1, 0.5), TS.label_smoothing_f32(logits, target, K - 1, 0.1, 0.5)
    TS.compare_rows(rows.detach(), spec[0], yard[0], "row_loss")
    TS.compare_rows(lg.grad, spec[1], yard[1], "dlogits")
    W, b, r8 = torch.randn(50, D, generator=g), torch.randn(50, generator=g), torch.randn(8, 50, generator=g)
    got = F.relu(F.linear(x[:8], W, b) + r8)
    TS.compare_rows(got, TS.linear_rows_spec(x[:8], W, b, r8, True), TS.linear_rows_f32(x[:8], W, b, r8, True), "linear")


def _rejected(got, ref, yardstick, what):
    with pytest.raises(AssertionError, match=what):
        TS.compare_rows(got, ref, yardstick, what)


def test_compare_rows_rejects_one_pass_variance():
    M, D = 24, 512
    _, x, r, gamma, beta, _ = _ln_inputs(M, D, False, 500, "offset")
    ref = TS.layernorm_spec(x, None, gamma, beta, EPS)
    yard = TS.layernorm_f32(x, None, gamma, beta, EPS)[0]
    TS.compare_rows(yard, ref, yard, "two passes")
    _rejected(TS.layernorm_f32(x, None, gamma, beta, EPS, one_pass=True)[0], ref, yard, "one pass")


@pytest.mark.parametrize("D", [252, 260, 2044])
def test_compare_rows_rejects_mean_over_padded_width(D):
    _, x, r, gamma, beta, _ = _ln_inputs(9, D, True, 510 + D)
    ref = TS.layernorm_spec(x, r, gamma, beta, EPS)
    yard = TS.layernorm_f32(x, r, gamma, beta, EPS)[0]
    _rejected(TS.layernorm_f32(x, r, gamma, beta, EPS, mean_count=(D + 255) // 256 * 256)[0], ref, yard, "padded mean")


def test_compare_rows_rejects_dgamma_without_last_float4():
    _, x, r, gamma, beta, dy = _ln_inputs(393, 516, True, 520)
    ref = TS.layernorm_bwd_spec(x, r, gamma, dy, EPS)[2]
    yard = TS.layernorm_bwd_f32(x, r, gamma, dy, EPS)[2]
    got = yard.clone()
    got[-4:] = 0.0
    _rejected(got, ref, yard, "dgamma")


def test_compare_rows_rejects_one_small_wrong_row():
    """The fault a whole-tensor max|err| / max|ref| cannot see: one row off by 1e-3 of itself among rows 100 times larger."""
    _, x, r, gamma, beta, dy = _ln_inputs(9, 96, False, 530)
    dy[:4] *= 100.0
    dy[5:] *= 100.0
    ref = TS.layernorm_bwd_spec(x, None, gamma, dy, EPS)[0]
    yard = TS.layernorm_bwd_f32(x, None, gamma, dy, EPS)[0]
    got = yard.clone()
    got[4] *= 1.0 + 1e-3
    whole = float((got.double() - ref).abs().max() / ref.abs().max())
    assert whole < 2e-5, "the old metric at its tolerance passes this tensor"
    _rejected(got, ref, yard, "dz")


@pytest.mark.parametrize("K,nc", [(512, 512), (513, 512), (17, 17)])
def test_compare_rows_rejects_smoothing_spread_over_K(K, nc):
    g = torch.Generator().manual_seed(540 + K)
    logits, target = torch.randn(6, K, generator=g), torch.randint(0, K, (6,), generator=g)
    ref = TS.label_smoothing_spec(logits, target, nc, 0.1, 1.0 / 6)
    yard = TS.label_smoothing_f32(logits, target, nc, 0.1, 1.0 / 6)
    got = TS.label_smoothing_f32(logits, target, nc, 0.1, 1.0 / 6, off=0.1 / K)
    _rejected(got[0], ref[0], yard[0], "row_loss")
    _rejected(got[1], ref[1], yard[1], "dlogits")


@pytest.mark.parametrize("K,nc,scale", [(17, 16, 1.0), (513, 512, 30.0)])
def test_compare_rows_rejects_gradient_that_takes_true_dist_to_sum_to_one(K, nc, scale):
    """(softmax - true_dist) is the gradient only where true_dist sums to 1, i.e. for K == num_classes: what
    label_smoothing_kernel wrote for every K until these tests."""
    g = torch.Generator().manual_seed(545 + K)
    logits, target = scale * torch.randn(6, K, generator=g), torch.randint(0, K, (6,), generator=g)
    ref = TS.label_smoothing_spec(logits, target, nc, 0.1, 1.0 / 6)[1]
    yard = TS.label_smoothing_f32(logits, target, nc, 0.1, 1.0 / 6)[1]
    _rejected(TS.label_smoothing_f32(logits, target, nc, 0.1, 1.0 / 6, unit_sum=True)[1], ref, yard, "dlogits")
    same = TS.label_smoothing_f32(logits, target, K, 0.1, 1.0 / 6, unit_sum=True)[1]
    TS.compare_rows(same, TS.label_smoothing_spec(logits, target, K, 0.1, 1.0 / 6)[1], same, "K == num_classes")


@pytest.mark.parametrize("K", [252, 260, 2044])
def test_compare_rows_rejects_linear_rows_without_the_k_tail(K):
    g = torch.Generator().manual_seed(550 + K)
    x, W, b = torch.randn(5, K, generator=g), torch.randn(50, K, generator=g), torch.randn(50, generator=g)
    ref, yard = TS.linear_rows_spec(x, W, b, None, False), TS.linear_rows_f32(x, W, b, None, False)
    cut = K - K % 256
    _rejected(TS.linear_rows_f32(x[:, :cut], W[:, :cut], b, None, False), ref, yard, "linear")


def test_compare_rows_rejects_non_finite_and_wrong_shape():
    ref = torch.ones(3, 4, dtype=torch.float64)
    yard = torch.ones(3, 4)
    got = yard.clone()
    got[1, 2] = float("nan")
    _rejected(got, ref, yard, "nan")
    with pytest.raises(AssertionError):
        TS.compare_rows(yard[:2], ref, yard, "shape")
    assert TS.row_error(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.float64)) == 0.0     # 0 / 2^-100, not 0 / 0


def test_row_kernels_refuse_unsupported_shapes_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    fake = 0x10000       # non-null, 16-byte aligned, never dereferenced on the host
    INVALID, UNSUPPORTED = -1, -4
    for D in (6, 2052):  # D % 4 != 0, D > 2048
        assert lib.isi_layernorm_f32(fake, None, fake, fake, fake, 4, D, EPS, None) == UNSUPPORTED
        assert b"D % 4 == 0 and D <= 2048" in lib.isi_last_error()
        assert lib.isi_layernorm_dropout_f32(fake, fake, fake, fake, fake, 4, D, EPS, 0.3, 1, None) == UNSUPPORTED
        assert lib.isi_layernorm_bwd_f32(fake, None, fake, fake, fake, fake, fake, fake, 4, D, EPS, None) == UNSUPPORTED
        assert lib.isi_layernorm_dropout_bwd_f32(fake, fake, fake, fake, fake, fake, fake, fake, fake, 4, D, EPS, 0.3, 1,
                                                 None) == UNSUPPORTED
    assert lib.isi_linear_rows_f32(fake, 96, fake, fake, None, 0, fake, 50, 9, 50, 96, 0, None) == UNSUPPORTED
    assert b"at most 8 rows" in lib.isi_last_error()
    assert lib.isi_linear_rows_f32(fake, 96, fake, fake, None, 0, fake, 50, 5, 50, 94, 0, None) == INVALID
    assert lib.isi_linear_rows_f32(fake, 98, fake, fake, None, 0, fake, 50, 5, 50, 96, 0, None) == INVALID
    for K in (1, 0):
        assert lib.isi_label_smoothing_loss_f32(fake, fake, fake, fake, 4, K, 17, 0.1, 0.25, None) == INVALID
    assert lib.isi_label_smoothing_loss_f32(fake, fake, fake, fake, 4, 2, 1, 0.1, 0.25, None) == INVALID
    # the workspace of the backward: two partial rows per block, 8 rows per block up to 1024 blocks
    assert lib.isi_layernorm_bwd_workspace_floats(392, 516) == 49 * 2 * 516
    assert lib.isi_layernorm_bwd_workspace_floats(8193, 64) == 1024 * 2 * 64
