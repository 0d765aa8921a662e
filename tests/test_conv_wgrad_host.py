"""What tests/test_conv_wgrad_gpu.py measures the weight-gradient kernels with, checked without a GPU: the float64
specifications of tests/tests_support.py against float64 autograd, the comparison against mutants of the float32
yardstick (each imitates a way csrc/conv_wgrad_f32.hip could be wrong and must be rejected under the bound of the mode it
imitates), the unmutated yardstick under every bound of every GPU case, and the refusals of the C-ABI that happen on the host."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import tests_support as TS

CASES = {TS.wgrad_case_id(c): c for c in TS.WGRAD_CASES}


def _case(name):
    return CASES[name]


# ------------------------------------------------------------------------------------------------- spec against autograd
@pytest.mark.parametrize("cfg", [
    # (C0, C1, Cout, k, stride, pad, transposed, groups, B, H, W)
    (3, 0, 5, 1, 1, 0, False, 1, 2, 5, 7), (4, 0, 6, 3, 1, 1, False, 1, 2, 5, 7), (4, 0, 6, 3, 2, 1, False, 1, 1, 7, 9),
    (4, 0, 6, 3, 1, 0, False, 1, 2, 5, 7), (2, 0, 3, 4, 2, 1, False, 1, 2, 6, 10), (2, 0, 3, 4, 2, 0, False, 1, 1, 7, 9),
    (3, 5, 4, 3, 1, 1, False, 1, 2, 5, 7), (6, 0, 4, 3, 1, 1, False, 2, 1, 5, 7), (2, 4, 6, 4, 2, 1, False, 2, 1, 7, 5),
    (1, 0, 1, 1, 2, 0, False, 1, 1, 3, 3), (5, 0, 3, 4, 2, 1, True, 1, 2, 3, 5), (4, 0, 6, 4, 2, 1, True, 2, 1, 5, 3),
])
def test_spec_equals_float64_autograd(cfg):
    c0, c1, cout, k, s, p, tr, groups, B, H, W = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn(B, c0, H, W, generator=g, dtype=torch.float64)
    x2 = torch.randn(B, c1, H, W, generator=g, dtype=torch.float64) if c1 else None
    xin = x if x2 is None else torch.cat([x, x2], 1)
    cin = c0 + c1
    if tr:
        w = torch.randn(cin, cout // groups, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(xin, w, b, stride=s, padding=p, groups=groups)
    else:
        w = torch.randn(cout, cin // groups, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xin, w, b, stride=s, padding=p, groups=groups)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    dw, db = TS.conv_wgrad_spec(x, x2, dy.permute(0, 2, 3, 1), k, s, p, tr, groups)
    assert dw.shape == w.shape and dw.dtype == torch.float64
    assert TS.row_error(TS.rows2d(dw), TS.rows2d(w.grad)) <= 1e-12
    assert TS.row_error(db, b.grad) <= 1e-12


@pytest.mark.parametrize("shape", [(6, 8, 1, 3, 5), (4, 3, 2, 4, 7)])
def test_four_phase_form_equals_the_spec(shape):
    """The phase decomposition and its unpacking (tap (ty, tx) of phase (py, px) = torch tap (3 - py - 2 ty, 3 - px - 2 tx))."""
    cin, cout, B, H, W = shape
    g = torch.Generator().manual_seed(7)
    x, dy = torch.randn(B, cin, H, W, generator=g), torch.randn(B, 2 * H, 2 * W, cout, generator=g)
    spec, _ = TS.conv_wgrad_spec(x, None, dy, 4, 2, 1, True)
    got = TS.convT_unpack_phases(TS.convT_phases_f32(x, dy, dtype=torch.float64), cin, cout)
    assert TS.row_error(TS.rows2d(got), TS.rows2d(spec)) <= 1e-12


def test_embed_sum_spec_equals_one_hot_product():
    g = torch.Generator().manual_seed(3)
    for N, D, K in ((1, 4, 32), (33, 8, 32), (500, 64, 64)):
        z = torch.randn(N, D, generator=g)
        idx = torch.randint(0, K, (N,), generator=g)
        want = z.double().t() @ F.one_hot(idx, K).double()
        got = TS.embed_sum_spec(z, idx, K)
        assert got.shape == (D, K) and got.dtype == torch.float64
        assert TS.row_error(got, want) <= 1e-12
        assert TS.row_error(TS.embed_sum_f32(z, idx, K), want) <= 8 * TS.ROW_OPS_FLOOR


def test_split_models_are_ordered_as_designed():
    """pieces = 2 truncates at ~2^-17 of a product, pieces = 3 far below one float32 ulp of the row; pair rounding is within
    2^-22 of the value (or 2^-26 absolute)."""
    c = _case("split-conv8to16k3s1p1-1x5x7-nhwc")
    r = TS.wgrad_case_refs(c)
    e2 = TS.row_error(TS.rows2d(r.model2), TS.rows2d(r.spec_dw))
    e3 = TS.row_error(TS.rows2d(r.model3), TS.rows2d(r.spec_dw))
    assert 2.0 ** -22 < e2 < 2.0 ** -15 and e3 < 2.0 ** -24, (e2, e3)
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1))
    assert bool(((TS.pair_round_f16(x) - x).abs() <= 2.0 ** -22 * x.abs() + 2.0 ** -26).all())   # (2^-26: a subnormal f16 lo piece)


# ------------------------------------------------------------------------------------- what the comparison accepts / rejects
def _bounds(c):
    """{flags: yardstick of that mode} for the weight gradient of a case."""
    r = TS.wgrad_case_refs(c)
    modes = (0, 2, 4) if c.vec else (0,)
    return {f: TS.conv_wgrad_yardstick(f, r.spec_dw, r.f32_dw, r.model2, r.model3) for f in modes}


@pytest.mark.parametrize("name", list(CASES))
def test_unmutated_yardstick_passes_every_bound(name):
    """The float32 evaluation of every GPU case lies inside the bound of every mode the case is run in: the inputs themselves
    do not exhaust a bound (the six-term mode's yardstick is its model, usually floored at one float32 ulp)."""
    c = _case(name)
    r = TS.wgrad_case_refs(c)
    for flags, yard in _bounds(c).items():
        TS.compare_rows(TS.rows2d(r.f32_dw), TS.rows2d(r.spec_dw), TS.rows2d(yard), f"{name} flags {flags} dW")   # (margin 8 in every mode)
        if flags:
            model = r.model2 if flags == 2 else r.model3
            TS.compare_rows(TS.rows2d(model), TS.rows2d(r.spec_dw), TS.rows2d(yard), f"{name} flags {flags} model dW")
    TS.compare_rows(r.f32_db, r.spec_db, r.f32_db, f"{name} db")


def _rejected(c, mutant_dw, flags_list, what):
    r = TS.wgrad_case_refs(c)
    bounds = _bounds(c)
    for flags in flags_list:
        with pytest.raises(AssertionError):
            TS.compare_rows(TS.rows2d(mutant_dw), TS.rows2d(r.spec_dw), TS.rows2d(bounds[flags]), f"{what} flags {flags}")


def _args(c):
    x, x2, dy = TS.wgrad_case_data(c)
    return (x, x2, dy, c.k, c.stride, c.pad, c.transposed)


def test_mutant_a_last_partial_chunk_dropped():
    c = _case("split-conv8to16k3s1p1-1x5x7-nhwc")                  # M = 35: the last M % 32 = 3 pixels
    keep = torch.arange(35) < 32
    _rejected(c, TS.conv_wgrad_f32_yardstick(*_args(c), pixels=keep)[0], (0, 2, 4), "last M % 32 pixels dropped")


def test_mutant_b_last_pixel_split_dropped():
    c = _case("split-conv64to128k3s1p1-2x9x37-nhwc")               # M = 666: splits of 11 and 10 chunks
    keep = torch.arange(666) < 11 * 32
    _rejected(c, TS.conv_wgrad_f32_yardstick(*_args(c), pixels=keep)[0], (0, 2, 4), "last pixel split dropped")


def test_mutant_c_border_clamped():
    c = _case("split-conv8to16k3s1p1-1x5x7-nhwc")
    _rejected(c, TS.conv_wgrad_f32_yardstick(*_args(c), clamp_border=True)[0], (0, 2, 4), "border taps clamped")


def test_mutant_d_sources_swapped():
    c = _case("scalar-conv6+10to16k3s1p1-1x5x7-nhwc")
    _rejected(c, TS.conv_wgrad_f32_yardstick(*_args(c), swap_sources=True)[0], (0,), "channel blocks of the sources swapped")
    c = _case("split-conv64+64to128k3s1p1-2x9x37-nhwc")
    _rejected(c, TS.conv_wgrad_f32_yardstick(*_args(c), swap_sources=True)[0], (0, 2, 4), "channel blocks of the sources swapped")


def test_mutant_e_bias_gradient_from_one_split():
    c = _case("split-conv64to128k3s1p1-2x9x37-nhwc")
    r = TS.wgrad_case_refs(c)
    db = TS.conv_wgrad_f32_yardstick(*_args(c), db_pixels=torch.arange(666) < 11 * 32)[1]
    with pytest.raises(AssertionError):
        TS.compare_rows(db, r.spec_db, r.f32_db, "db from one split")


@pytest.mark.parametrize("name", ["split-conv8to16k3s1p1-1x5x7-nhwc", "split-conv64to128k3s1p1-2x9x37-nhwc",
                                  "split-convT128to64k4s2p1-1x3x5-nhwc"])
def test_mutant_f_operand_carried_as_hi_only(name):
    """A two-term product (one operand without its lo piece) must not fit under the three-term bound."""
    c = _case(name)
    _rejected(c, TS.conv_wgrad_f32_yardstick(*_args(c), x_hi_only=True)[0], (2,), "operand as hi only")


@pytest.mark.parametrize("name", ["split-conv8to16k3s1p1-1x5x7-nhwc", "split-conv64to128k3s1p1-2x9x37-nhwc"])
def test_mutant_g_six_term_model_without_lo(name):
    c = _case(name)
    a = _args(c)
    _rejected(c, TS.conv_wgrad_split_model(*a, pieces=3, drop_lo=True), (4,), "six-term model without its lo pieces")


@pytest.mark.parametrize("shape", [s for s in TS.WGRAD_PHASE_CASES if s[2] == 1])
def test_mutant_h_phases_share_one_padding(shape):
    cin, cout, B, H, W, vec = shape
    x, dy = TS.wgrad_phase_case_data(shape)
    spec, _ = TS.conv_wgrad_spec(x, None, dy, 4, 2, 1, True)
    good = TS.convT_unpack_phases(TS.convT_phases_f32(x, dy), cin, cout)
    bad = TS.convT_unpack_phases(TS.convT_phases_f32(x, dy, pad_of=lambda p: 1), cin, cout)
    a = (x, None, dy, 4, 2, 1, True)
    yards = {0: good}
    if vec:
        m2, m3 = TS.conv_wgrad_split_model(*a, pieces=2), TS.conv_wgrad_split_model(*a, pieces=3)
        yards = {f: TS.conv_wgrad_yardstick(f, spec, good, m2, m3) for f in (0, 2, 4)}
    for flags, yard in yards.items():
        TS.compare_rows(TS.rows2d(good), TS.rows2d(spec), TS.rows2d(yard), f"four-phase yardstick flags {flags}")
        with pytest.raises(AssertionError):
            TS.compare_rows(TS.rows2d(bad), TS.rows2d(spec), TS.rows2d(yard), f"pad = 1 in both phases, flags {flags}")


# ------------------------------------------------------------------------------------------------ refusals on the host
FAKE = 0x10000       # non-null, 16-byte aligned, never dereferenced on the host


def _src(Cc, H, W, ptr=FAKE):
    from interactive_spectrogram_inpainting import _hip
    return _hip.isi_src(ptr, Cc, H * W * Cc, 1, W * Cc, Cc)


def test_weight_gradient_refusals_need_no_gpu():
    """Every refusal below is decided before any launch (no device is touched).  The batch-count check (`nz` outside 1..255)
    belongs to the internal batched entry the attention backward calls; no exported function passes an `nz`, so it cannot be
    reached from here."""
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
    B, H, W, cin, cout = 1, 2, 33, 64, 64
    s0 = _src(cin, H, W)
    nws = L.isi_conv_wgrad_workspace_floats(cout, 9 * cin, B * H * W, 1)
    plain = lambda *a: L.isi_conv_wgrad_f32(*a)
    # null pointers: source, dY, dW, workspace
    assert plain(None, None, FAKE, FAKE, None, FAKE, nws, B, H, W, cout, 3, 3, 1, 1, 2, None) == INVALID
    assert b"null" in L.isi_last_error()
    assert plain(C.byref(_src(cin, H, W, ptr=None)), None, FAKE, FAKE, None, FAKE, nws, B, H, W, cout, 3, 3, 1, 1, 2, None) == INVALID
    assert plain(C.byref(s0), None, None, FAKE, None, FAKE, nws, B, H, W, cout, 3, 3, 1, 1, 2, None) == INVALID
    assert plain(C.byref(s0), None, FAKE, None, None, FAKE, nws, B, H, W, cout, 3, 3, 1, 1, 2, None) == INVALID
    assert plain(C.byref(s0), None, FAKE, FAKE, None, None, nws, B, H, W, cout, 3, 3, 1, 1, 2, None) == INVALID
    # a workspace one float short of what this launch needs, in each precision mode; the sizer covers every mode
    for flags in (0, 2, 4):
        # (one split of the 128 x 128 tile at M = 66: nchunks / 8 = 0 -> 1 split: [Cout][Kpad] partials + [Cout] bias partials)
        need = cout * 9 * cin + cout
        assert need <= nws
        assert plain(C.byref(s0), None, FAKE, FAKE, FAKE, FAKE, need - 1, B, H, W, cout, 3, 3, 1, 1, flags, None) == WORKSPACE
        assert b"workspace" in L.isi_last_error()
    # pair-format sources on a launch the halo-staged kernel does not take (OW = 33; six-term products; fp32 pipe)
    assert L.isi_conv_wgrad_halo_route(cout, cin, 0, 3, 3, 1, 1, H, W) == 0
    assert L.isi_conv_wgrad_halo_route(cout, cin, 0, 3, 3, 1, 1, H, 32) == 1
    for flags, w in ((2 | 32, W), (2 | 64, W), (4 | 32, 32), (0 | 32, 32)):
        s = _src(cin, H, w)
        assert plain(C.byref(s), None, FAKE, FAKE, None, FAKE, nws, B, H, w, cout, 3, 3, 1, 1, flags, None) == UNSUPPORTED
        assert b"pair" in L.isi_last_error()
    # torch-layout output of the four-phase transposed form
    nws_t = L.isi_conv_wgrad_workspace_floats(cout, 4 * cin, B * H * W, 4)
    rc = L.isi_conv_wgrad_torch_f32(C.byref(s0), None, FAKE, FAKE, cin, None, FAKE, nws_t, B, H, W, cout, 4, 4, 2, 1, 1 | 2, None)
    assert rc == UNSUPPORTED and b"torch-layout" in L.isi_last_error()
    assert L.isi_conv_wgrad_torch_f32(C.byref(s0), None, FAKE, FAKE, 0, None, FAKE, nws, B, H, W, cout, 3, 3, 1, 1, 2, None) == INVALID
    # the transposed form is k4 s2 p1 only; an empty output
    assert plain(C.byref(s0), None, FAKE, FAKE, None, FAKE, nws_t, B, H, W, cout, 3, 3, 1, 1, 1, None) == UNSUPPORTED
    assert plain(C.byref(s0), None, FAKE, FAKE, None, FAKE, nws, B, 2, 2, cout, 4, 4, 2, 0, 2, None) == INVALID
    # deferred form without a job list
    assert L.isi_conv_wgrad_deferred_f32(C.byref(s0), None, FAKE, FAKE, cin, None, FAKE, nws, B, H, W, cout, 3, 3, 1, 1, 2, None,
                                         None, None) == INVALID


def test_embed_sum_and_pad_channels_refusals_need_no_gpu():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    big = 1 << 30
    assert L.isi_vq_embed_sum_f32(FAKE, FAKE, FAKE, FAKE, big, 100, 6, 32, None) == -1          # D % 4
    assert b"D % 4" in L.isi_last_error()
    assert L.isi_vq_embed_sum_f32(FAKE, FAKE, FAKE, FAKE, big, 100, 64, 48, None) == -1         # K % 32
    assert L.isi_vq_embed_sum_f32(FAKE, FAKE, FAKE, FAKE, big, 0, 64, 32, None) == -1           # no vectors
    for null_at in range(4):
        ptrs = [FAKE] * 4
        ptrs[null_at] = None
        assert L.isi_vq_embed_sum_f32(*ptrs, big, 100, 64, 32, None) == -1
    # N = 4099, D = 64, K = 512: 16 splits of [D][K] partials (tests/test_conv_wgrad_gpu.py); one float short
    assert L.isi_vq_embed_sum_f32(FAKE, FAKE, FAKE, FAKE, 16 * 64 * 512 - 1, 4099, 64, 512, None) == -3
    assert L.isi_vq_embed_sum_workspace_floats(64, 512, 4099) >= 16 * 64 * 512
    s = _src(5, 2, 2)
    assert L.isi_pad_channels4_f32(C.byref(s), FAKE, 1, 2, 2, None) == -1                       # C > 4
    s = _src(2, 2, 2)
    assert L.isi_pad_channels4_f32(None, FAKE, 1, 2, 2, None) == -1
    assert L.isi_pad_channels4_f32(C.byref(s), None, 1, 2, 2, None) == -1
    assert L.isi_pad_channels4_f32(C.byref(s), FAKE + 4, 1, 2, 2, None) == -1                   # output not 16-byte aligned
