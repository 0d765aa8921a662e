"""What tests/test_linear_gemm_gpu.py relies on, shown without a GPU: the float64 specification of the linear layers' GEMM
(tests_support.linear_spec) against float64 autograd, the integer replica of the dropout mask, the Python mirror of the tile
route against the library's own answer, the comparison `tests_support.linear_hold` accepting the float32 evaluation at
every small GPU shape and rejecting every mutant on the list below, and the argument refusals of isi_linear_f32 /
gemm_split_f32 (fake pointers: each returns before anything touches a device)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tests_support as TS

SMALL, WIDE = TS.linear_cases(256)
MODES = ("bf16", "f16")


def _id(c):
    return f"{c.M}x{c.N}x{c.K}"


def _refs(c):
    """(data, float64 product, float32 product, {mode: three-term model}) of a case: computed once, left unchanged."""
    r = TS.linear_case_refs(c.M, c.N, c.K)
    return (r.x, r.W, r.bias, r.res, r.gate), r.prod64, r.prod32, r.model


def _expect(c, mode, which, ldo=None):
    (x, W, bias, res, gate), p64, p32, model = _refs(c)
    e = TS.linear_epilogue_args(which, c.M, c.N, c.N + 3 if ldo is None else ldo, bias, res, gate)
    return e, TS.linear_expect(p64, p32, model[mode], c.tail, *e)


# ------------------------------------------------------------------------------------------------------------ the spec
@pytest.mark.parametrize("relu,gated,dropped", [(False, False, False), (True, False, False), (True, True, False),
                                                (True, False, True), (True, True, True), (False, True, True)])
def test_linear_spec_equals_float64_autograd(relu, gated, dropped):
    """Values, and the input gradient as the project computes it: the next layer's input-gradient GEMM dY W2 gated by this
    layer's output (> 0 where the ReLU, the gate and the mask all pass) and scaled by gate_scale / (1 - p) -- linear_spec
    with a gate --, then the plain product with W."""
    g = torch.Generator().manual_seed(3)
    M, N, K, p, gs = 9, 7, 5, 0.5, 1.5                    # (gate_scale / (1 - p) = 3: exact in float32)
    x = torch.randn(M, K, generator=g, dtype=torch.float64, requires_grad=True)
    W, b, res = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((N, K), (N,), (M, N)))
    gate = TS.gate_data(M * N, g)[1].reshape(M, N) if gated else None
    keep = TS.dropout_keep_mask(77, M, N, N + 3, p) if dropped else None
    y = torch.nn.functional.linear(x, W, b) + res
    y = torch.relu(y) if relu else y
    if gated:
        y = y * (gate > 0).double() * gs
    if dropped:
        y = y * keep.double() / (1.0 - p)
    W2 = torch.randn(4, N, generator=g, dtype=torch.float64)             # the layer behind: its input-gradient GEMM is gated
    dy = torch.randn(M, 4, generator=g, dtype=torch.float64)
    torch.nn.functional.linear(y, W2).backward(dy)
    spec = TS.linear_spec(x, W, b, res, relu, gate, gs, keep, p if dropped else 0.0)
    assert torch.allclose(spec, y.detach(), rtol=1e-14, atol=1e-14)
    if relu:    # (without the ReLU the output's sign is not the mask)
        scale = (gs if gated else 1.0) / ((1.0 - p) if dropped else 1.0)
        dpre = TS.linear_spec(dy, W2.t(), None, None, False, y.detach(), scale, None, 0.0)
        dx = TS.linear_spec(dpre, W.t(), None, None, False)
        assert torch.allclose(dx, x.grad, rtol=1e-13, atol=1e-13)
    # the float32 evaluation is the same function
    f32 = TS.linear_f32(x, W, b, res, relu, gate, gs, keep, p if dropped else 0.0)
    assert f32.dtype == torch.float32 and torch.allclose(f32.double(), spec, rtol=1e-5, atol=1e-5)


def test_split_models_are_three_terms_of_an_exact_split():
    """hi + lo restores the operand (to 2^-16 of it in bf16, 2^-22 in f16 pieces), and the models differ from the exact
    product by the lo.lo term they leave out."""
    g = torch.Generator().manual_seed(5)
    x, W = torch.randn(64, 128, generator=g), torch.randn(48, 128, generator=g) / 128 ** 0.5
    exact = x.double() @ W.double().t()
    for mode, (xh, xl), (wh, wl), s, tol in (("bf16", TS.bf16_pieces(x, 2), TS.bf16_pieces(W, 2), 1.0, 2.0 ** -16),
                                              ("f16", TS.f16_pieces(x, 4.0), TS.f16_pieces(W, 1024.0), 4096.0, 2.0 ** -21)):
        sx, sw = (4.0, 1024.0) if mode == "f16" else (1.0, 1.0)
        assert float(((xh + xl) / sx - x.double()).abs().max() / x.abs().max()) <= tol
        assert float(((wh + wl) / sw - W.double()).abs().max() / W.abs().max()) <= tol
        rest = (xh + xl) @ (wh + wl).t() / s - xl @ wl.t() / s
        assert torch.allclose(TS.linear_split_model(x, W, mode), rest, rtol=0, atol=1e-12)
        assert TS.row_error(TS.linear_split_model(x, W, mode), exact) < 8 * tol
        for drop in ("hi_lo", "lo_hi"):
            assert TS.row_error(TS.linear_split_model(x, W, mode, drop=drop), exact) > 30 * tol


# ------------------------------------------------------------------------------------------------------------ the mask
def _keep_scalar(seed, idx, thresh):
    """dropout_keep of csrc/isi_internal.h, one element, Python integers."""
    m = 0xFFFFFFFF
    h = idx & m
    h ^= h >> 16
    h = h * 0x7FEB352D & m
    h ^= seed & m
    h ^= h >> 15
    h ^= seed >> 32 & m
    h = h * 0x846CA68B & m
    h ^= h >> 16
    return h >= thresh


def test_dropout_keep_mask():
    assert TS.dropout_thresh(0.25) == 2 ** 30
    assert TS.dropout_thresh(0.0) == 1 and TS.dropout_thresh(1.0) == 0xFFFFFFFF and TS.dropout_thresh(1e-12) == 1
    assert TS.dropout_thresh(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32)
    seed = TS.LINEAR_SEEDS[0]
    for p in (0.25, 0.1, 0.5):
        keep = TS.dropout_keep_mask(seed, 1024, 1024, 1024, p)          # 2^20 consecutive indices
        assert abs(float(keep.double().mean()) - (1.0 - p)) < 0.005
    a = TS.dropout_keep_mask(seed, 64, 200, 203, 0.25)
    assert not torch.equal(a, TS.dropout_keep_mask(seed + 2 ** 32, 64, 200, 203, 0.25)), "the high word must count"
    assert not torch.equal(a, TS.dropout_keep_mask(seed ^ 1, 64, 200, 203, 0.25))
    assert not torch.equal(a, TS.dropout_keep_mask(seed, 64, 200, 200, 0.25)), "the index is m ldo + n"
    assert not torch.equal(a, TS.dropout_keep_mask(seed, 64, 200, 203, 0.25, high_word=False))
    assert torch.equal(a, TS.dropout_keep_mask(seed, 64, 200, 203, 0.25))
    for m, n in ((0, 0), (1, 0), (17, 199), (63, 5)):                    # the vectorised form against the scalar one
        assert bool(a[m, n]) == _keep_scalar(seed, m * 203 + n, 2 ** 30)
    # the index wraps at 32 bits, as the kernel's
    far = TS.dropout_keep_mask(seed, 2, 8, 2 ** 32 + 5, 0.25)
    assert torch.equal(far[1], TS.dropout_keep_mask(seed, 2, 8, 5, 0.25)[1])


# ----------------------------------------------------------------------------------------------------------- the route
def _route(tile, tail=0):
    return tile | tail << 8


def test_linear_route_at_256_compute_units():
    for c in SMALL + WIDE:
        assert TS.linear_route(c.M, c.N, c.K, 256, dict(c.knobs).get("ISI_GEMM_NARROW_BELOW", 0),
                               dict(c.knobs).get("ISI_GEMM_NO_WIDE", 0)) == _route(c.tile, c.tail), c
    # the training workload's linear layers: M = 8 x 1025 rows, K = 512
    for N, tile in ((512, 2), (1024, 3), (1536, 2), (2048, 4)):
        assert TS.linear_route(8200, N, 512, 256) == _route(tile, 8), N
    # outside the kernel
    for M, N, K in ((255, 64, 128), (256, 32, 128), (256, 64, 96), (256, 64, 144)):
        assert TS.linear_route(M, N, K, 256) == 0
    # the wide shapes follow the CU count
    for cus in (64, 128, 304):
        small, wide = TS.linear_cases(cus)
        for c in small + wide:
            assert TS.linear_route(c.M, c.N, c.K, cus, dict(c.knobs).get("ISI_GEMM_NARROW_BELOW", 0),
                                   dict(c.knobs).get("ISI_GEMM_NO_WIDE", 0)) == _route(c.tile, c.tail), (cus, c)


def test_library_route_equals_the_mirror():
    """isi_linear_route with the CU count given by a knob (no device is asked): the mirror's answer at every case, at the
    workload's shapes and over a grid of shapes and knob values."""
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    shapes = [(c.M, c.N, c.K) for c in SMALL + WIDE] + [(8200, N, 512) for N in (512, 1024, 1536, 2048)]
    shapes += [(M, N, 128) for M in (255, 256, 1023, 1024, 1025, 1040, 1041, 4100, 16384, 32768) for N in (32, 33, 64, 128, 256, 384, 512)]
    shapes += [(256, 64, 96), (256, 64, 144), (512, 512, 64)]
    for cus in (256, 64):
        with _hip.knob("ISI_CU_COUNT", cus):
            for nb, nw in ((0, 0), (1, 0), (0, 1), (0, 2), (1000, 0)):
                with _hip.knob("ISI_GEMM_NARROW_BELOW", nb), _hip.knob("ISI_GEMM_NO_WIDE", nw):
                    for M, N, K in shapes:
                        for flags in (2, 8, 8 | 16, 2 | 256):
                            assert L.isi_linear_route(M, N, K, flags) == TS.linear_route(M, N, K, cus, nb, nw), (cus, nb, nw, M, N, K)
            assert L.isi_linear_route(1024, 512, 128, 0) == 0 and L.isi_linear_route(1024, 512, 128, 4) == 0   # fp32, six-term
            with _hip.knob("ISI_NO_GEMM_KERNEL", 1):
                assert L.isi_linear_route(1024, 512, 128, 2) == 0


# ------------------------------------------------------------------------------------------------------ the comparison
@pytest.mark.parametrize("c", SMALL, ids=_id)
def test_float32_evaluation_passes_its_own_comparison(c):
    (x, W, bias, res, gate), _, _, _ = _refs(c)
    for mode in MODES:
        for which in TS.LINEAR_EPILOGUES:
            e, exp = _expect(c, mode, which)
            checks = TS.linear_hold(TS.linear_f32(x, W, *e), exp, f"{_id(c)} {mode} {which}")
            assert len(checks) == (2 if c.tail else 1) and all(k.ratio <= 1.0 for k in checks)
            # ... and so does the mode's own model (what a correct kernel computes, but for its fp32 accumulation)
            model = TS._linear_epilogue(_refs(c)[3][mode], *e)[0]
            if c.tail:
                model[-c.tail:] = TS.linear_f32(x, W, *e)[-c.tail:].double()
            TS.linear_hold(model.float(), exp, f"{_id(c)} {mode} {which} model")


def _case(M, N, K):
    return next(c for c in SMALL if (c.M, c.N, c.K) == (M, N, K))


def _rejected(got, exp, what):
    with pytest.raises(AssertionError):
        TS.linear_hold(got, exp, what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("drop", ["hi_lo", "lo_hi"])
def test_a_dropped_cross_term_is_rejected(mode, drop):
    for c in (_case(300, 200, 128), _case(385, 256, 160)):
        (x, W, *_), _, _, _ = _refs(c)
        for which in ("bias", "all"):
            e, exp = _expect(c, mode, which)
            got = TS._linear_epilogue(TS.linear_split_model(x, W, mode, drop=drop), *e)[0].float()
            _rejected(got, exp, f"{mode} without {drop}")


@pytest.mark.parametrize("mutant", ["skip_last_chunk", "repeat_chunk"])
def test_a_wrong_last_chunk_is_rejected(mutant):
    for c in (_case(257, 72, 160), _case(256, 40, 128), _case(256, 128, 128)):     # 5 and 4 chunks
        (x, W, *_), _, _, _ = _refs(c)
        for mode in MODES:
            e, exp = _expect(c, mode, "bias+res+relu")
            _rejected(TS.linear_f32(x, W, *e, **{mutant: True}), exp, mutant)


def test_wrong_strides_are_rejected():
    """Rows of x read at stride K, the residual at stride N, where the buffers have ldx = K + 32 (from column 16) and
    ldr = N + 4; the gaps hold finite values here (NaN in the GPU test), so the mutant's result is wrong, not NaN."""
    c = _case(300, 200, 128)
    (x, W, bias, res, gate), _, _, _ = _refs(c)
    g = torch.Generator().manual_seed(1)
    xw = torch.randn(c.M, c.K + 32, generator=g)
    xw[:, 16:16 + c.K] = x
    rw = torch.randn(c.M, c.N + 4, generator=g)
    rw[:, :c.N] = res
    for mode in MODES:
        e, exp = _expect(c, mode, "bias+res+relu")
        TS.linear_hold(TS.linear_f32(xw[:, 16:16 + c.K], W, bias, rw[:, :c.N], *e[2:]), exp, "views")
        _rejected(TS.linear_f32(x, W, *e, x_dense=(xw, 16)), exp, "x at stride K")
        _rejected(TS.linear_f32(x, W, *e, res_dense=(rw, 0)), exp, "residual at stride N")


@pytest.mark.parametrize("c", [_case(300, 200, 128), _case(1030, 192, 128), _case(1027, 128, 128)], ids=_id)
def test_a_wrong_mask_is_rejected(c):
    (x, W, bias, res, gate), _, _, _ = _refs(c)
    ldo, seed, p = c.N + 3, TS.LINEAR_SEEDS[0], TS.LINEAR_DROP_P
    for which in ("relu+dropout", "all"):
        e, exp = _expect(c, "f16", which)
        for what, keep in (("index m N + n", TS.dropout_keep_mask(seed, c.M, c.N, c.N, p)),
                           ("high word ignored", TS.dropout_keep_mask(seed, c.M, c.N, ldo, p, high_word=False)),
                           ("low word only of another seed", TS.dropout_keep_mask(TS.LINEAR_SEEDS[1], c.M, c.N, ldo, p))):
            _rejected(TS.linear_f32(x, W, *e[:5], keep, p), exp, what)
        _rejected(TS.linear_f32(x, W, *e, keep_unscaled=True), exp, "kept values not scaled")
        if c.tail:    # the mask wrong in the tail rows alone
            keep = e[5].clone()
            keep[-c.tail:] = TS.dropout_keep_mask(seed, c.M, c.N, c.N, p)[-c.tail:]
            _rejected(TS.linear_f32(x, W, *e[:5], keep, p), exp, "tail rows: index m N + n")


def test_a_wrong_gate_is_rejected():
    c = _case(300, 200, 128)
    (x, W, bias, res, gate), _, _, _ = _refs(c)
    assert int((gate == 0).sum()) > 100 and bool((gate[0, :2] == 0).all()) and bool(torch.signbit(gate[0, 1]))   # +0.0 and -0.0
    for mode in MODES:
        for which in ("gate", "all"):
            e, exp = _expect(c, mode, which)
            _rejected(TS.linear_f32(x, W, *e, gate_unscaled=True), exp, "gated value not scaled")
        e, exp = _expect(c, mode, "gate")
        _rejected(TS.linear_f32(x, W, *e, gate_ge=True), exp, "gate >= 0")


@pytest.mark.parametrize("c", [c for c in SMALL if c.tail], ids=_id)
def test_single_term_tail_rows_are_rejected(c):
    """Tail rows are plain fp32 dot products: single-term bf16 products there fail the tail block's float32 yardstick, and
    only that block."""
    (x, W, bias, res, gate), _, _, _ = _refs(c)
    for which in ("bias", "all"):
        e, exp = _expect(c, "bf16", which)
        got = TS.linear_f32(x, W, *e)
        got[-c.tail:] = TS.linear_f32(x, W, *e, tail_bf16=True)[-c.tail:]
        with pytest.raises(AssertionError, match="tail rows"):
            TS.linear_hold(got, exp, "bf16 tail")
        # the three-term model in the tail rows passes (it is fp32-grade there), a NaN row does not
        got = TS.linear_f32(x, W, *e)
        got[-1, 3] = float("nan")
        _rejected(got, exp, "NaN")


# ------------------------------------------------------------------------------------------------------- the refusals
def _args(M=256, N=64, K=128, **kw):
    from interactive_spectrogram_inpainting import _hip
    fake = 0x10000                 # non-null, 16-byte aligned, never dereferenced on the host
    a = _hip.isi_linear_args()
    a.x, a.packed_w, a.out, a.bias = fake, fake, fake, fake
    a.ldx, a.ldo, a.M, a.N, a.K, a.flags = K, N, M, N, K, 8
    a.gate_scale = 1.0
    for k, v in kw.items():
        if k in ("residual", "gate"):
            v = fake if v else None
        setattr(a, k, v)
    return a


def test_linear_refusals_need_no_device():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    INVALID, UNSUPPORTED = -1, -4
    run = lambda **kw: L.isi_linear_f32(C.byref(_args(**kw)), None)
    # a row stride shorter than its row
    assert run(ldx=124) == INVALID and b"stride" in L.isi_last_error()
    assert run(ldo=63) == INVALID
    assert run(residual=True, ldr=63) == INVALID
    assert run(residual=True, ldr=0) == INVALID
    assert run(gate=True, ldg=63) == UNSUPPORTED
    # dropout probabilities
    assert run(drop_p=-0.5) == INVALID and b"dropout" in L.isi_last_error()
    assert run(drop_p=float("nan")) == INVALID
    assert run(drop_p=1.0) == UNSUPPORTED and run(drop_p=1.5) == UNSUPPORTED
    # spans: at most 2^30 - 4 elements.  (M - 1) ldo + N = 2^30 exactly: the byte count would wrap to 0 and every store be dropped
    assert 256 * 4194303 + 256 == 2 ** 30
    assert run(M=257, N=256, ldo=4194303) == UNSUPPORTED and b"4 GiB" in L.isi_last_error()
    assert run(M=257, N=256, ldo=4194303, drop_p=0.25) == UNSUPPORTED
    # ... and one to three elements less still reaches beyond the out-of-range offset 2^32 - 16
    assert run(M=257, N=253, ldo=4194303) == UNSUPPORTED
    assert run(M=257, N=256, K=128, ldx=4194304) == UNSUPPORTED            # x: 256 * 2^22 + 128
    assert run(M=257, N=256, residual=True, ldr=4194303) == UNSUPPORTED
    assert run(M=257, N=256, ldo=256, gate=True, ldg=4194303) == UNSUPPORTED
    assert run(M=256, N=2 ** 23, K=128, ldo=2 ** 23) == UNSUPPORTED         # N K = 2^30 (and the output with it)
    # shapes outside the kernel, as before
    assert run(M=255) == UNSUPPORTED and run(K=96, ldx=96) == UNSUPPORTED and run(N=32, ldo=32) == UNSUPPORTED
    assert run(ldx=130) == UNSUPPORTED                                      # rows of x not 16-byte aligned
    assert L.isi_linear_f32(None, None) == INVALID


def test_convolution_span_of_exactly_4_gib_is_refused():
    """conv2d_f32 / conv_transpose2d_k4s2_f32: an extent of exactly 2^30 elements (its byte count wraps to 0) is refused
    like a larger one, before any launch."""
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    fake = 0x10000
    sw = 2 ** 30 - 4                                       # extent = (C - 1) + (W - 1) sw + 1 = 2^30 for C = 4, W = 2
    big, small = (fake, 0, 1, 0, sw), (fake, 0, 1, 0, 4)
    for s, d in ((big, small), (small, big)):
        src, dst = _hip.isi_src(s[0], 4, *s[1:]), _hip.isi_dst(*d)
        assert L.isi_conv2d_f32(C.byref(src), None, fake, None, None, C.byref(dst), 1, 1, 2, 4, 1, 1, 1, 0, 0, None) == -4
        assert b"4 GiB" in L.isi_last_error()
    src, res, dst = _hip.isi_src(fake, 4, *small[1:]), _hip.isi_src(fake, 4, *big[1:]), _hip.isi_dst(*small)
    assert L.isi_conv2d_f32(C.byref(src), None, fake, None, C.byref(res), C.byref(dst), 1, 1, 2, 4, 1, 1, 1, 0, 0, None) == -4
    # transposed: input [1, 4, 1, 2]; output [1, 4, 2, 4] of extent 3 + sh + 3 * 4 + 1 = 2^30
    src = _hip.isi_src(fake, 4, 0, 1, 0, sw)
    dst = _hip.isi_dst(fake, 0, 1, 8, 4)
    assert L.isi_conv_transpose2d_k4s2_f32(C.byref(src), fake, None, C.byref(dst), 1, 1, 2, 4, 0, None) == -4
    assert b"4 GiB" in L.isi_last_error()
    src, dst = _hip.isi_src(fake, 4, 0, 1, 0, 4), _hip.isi_dst(fake, 0, 1, 2 ** 30 - 16, 4)
    assert L.isi_conv_transpose2d_k4s2_f32(C.byref(src), fake, None, C.byref(dst), 1, 1, 2, 4, 0, None) == -4
