"""The convolution weight-gradient kernels of csrc/conv_wgrad_f32.hip against the float64 specification of
tests/tests_support.py, on every route of the dispatcher `conv_wgrad_batched_f32` and in every precision mode:
conv_wgrad_f32_kernel (vectorised and scalar gather), conv_wgrad_split_kernel<2|3> in its four tiles and its one-hot form
(isi_vq_embed_sum_f32), conv_wgrad_halo_kernel (fp32 and pair-format sources), the four-phase transposed form, the
reductions (torch layout, deferred jobs, packed) and isi_pad_channels4_f32.

Every comparison is `tests_support.compare_rows`, per output channel: the kernel may be 8 times as far from the float64
spec as the yardstick of its mode (tests_support.conv_wgrad_yardstick: the float32 evaluation on the CPU for the fp32 pipe,
the worse of that and the three-term model for flags 2, the six-term model for flags 4).  Outputs written in place lie
inside NaN buffers whose guards must keep their bits; every tensor the glue allocates itself (workspace, packed gradient,
padded source) starts as NaN and, in a second run, as zeros: the results must not differ by a bit.
tests/test_conv_wgrad_host.py shows, without a GPU, what the comparison accepts and rejects.

A recording aid, not a check: with ISI_WGRAD_RECORD=<file> in the environment every comparison's error, yardstick and ratio
are written there when the module ends, with the module's wall time (profiles/wgrad_checks.txt is such a run)."""
import contextlib
import ctypes as C
import os
import time

import pytest
import torch

import tests_support as TS
from test_prior_gpu import _dev

pytestmark = pytest.mark.gpu

PAD = 64                       # floats of NaN before and behind every guarded buffer (16-byte alignment stays)
RECORD = []                    # (case, route, flags, RowCheck)
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    t0 = time.time()
    yield
    path = os.environ.get("ISI_WGRAD_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# kernel error, yardstick of the mode (floored at 2^-23) and their ratio against the float64 spec, per comparison of\n"
                f"# tests/test_conv_wgrad_gpu.py; metric and bound: tests_support.compare_rows (ratio <= {TS.ROW_OPS_MARGIN:g}).  Worst ratio first.\n"
                f"# wall time of the file, reference computations on the CPU included: {time.time() - t0:.1f} s\n")
        worst = {}
        for case, route, flags, c in RECORD:
            worst[route] = max(worst.get(route, 0.0), c.ratio)
        for route in sorted(worst):
            f.write(f"# largest ratio, {route}: {worst[route]:.3f}\n")
        for case, route, flags, c in sorted(RECORD, key=lambda r: -r[3].ratio):
            f.write(f"{c.ratio:8.3f}  err {c.err:.3e}  yardstick {c.yardstick:.3e}  {route} flags {flags}  {case} {c.what}\n")


def _check(case, route, flags, got, ref, yardstick, what):
    got = TS.rows2d(got.detach().cpu())
    ref, yardstick = TS.rows2d(ref), TS.rows2d(yardstick)
    err, yard = TS.row_error(got, ref), max(TS.row_error(yardstick, ref), TS.ROW_OPS_FLOOR)
    print(f"{case} {route} flags {flags} {what}: err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    RECORD.append((case, route, flags, TS.RowCheck(what, err, yard, err / yard)))          # (recorded whether it passes or not)
    TS.compare_rows(got, ref, yardstick, f"{case} {route} flags {flags} {what}")


class Out:
    """A dense tensor of `shape` inside a flat NaN buffer with PAD floats of guard on either side."""

    def __init__(self, shape, dev, fill=NAN):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((PAD + n + PAD,), NAN, dtype=torch.float32, device=dev)
        self.view = self.buf[PAD:PAD + n].view(*shape)
        self.view.fill_(fill)
        self.n = n
        self.bits = self.buf.view(torch.int32).clone()

    def intact(self):
        now = self.buf.view(torch.int32)
        return bool(torch.equal(now[:PAD], self.bits[:PAD]) and torch.equal(now[PAD + self.n:], self.bits[PAD + self.n:]))


@contextlib.contextmanager
def _fresh_memory_holds(value):
    """While active, every floating-point tensor torch.empty returns starts filled with `value`: the workspace, the packed
    gradient and the padded source that vqvae/_train.py allocates for a launch.  A launch that allocated nothing this way
    (the glue allocating by another call) would leave the property untested: that is an error here."""
    real, calls = torch.empty, [0]

    def filled(*a, **k):
        t = real(*a, **k)
        if not t.is_floating_point():
            return t
        calls[0] += 1
        return t.fill_(value)
    torch.empty = filled
    try:
        yield
    finally:
        torch.empty = real
    assert calls[0] >= 1, "the launch allocated no workspace through torch.empty: nothing was poisoned"


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# --------------------------------------------------------------------------------------------- through vqvae/_train.py
def _device_operands(c, dev):
    """(x, x2, dy_nhwc) as vqvae/_train.py conv_wgrad takes them: [B, C, H, W] views of channels-last storage ("nchw": dense
    NCHW storage; "pair": PairOnly), dY dense -- for a transposed layer a channel slice of a wider NaN tensor."""
    from interactive_spectrogram_inpainting.vqvae import _ops, _train
    x, x2, dy = TS.wgrad_case_data(c)

    def src(t):
        if t is None:
            return None
        if c.layout == "nchw":
            return t.to(dev).contiguous()
        d = t.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        return _train.PairOnly(_ops.pair_encode(d)) if c.layout == "pair" else d
    if c.transposed:
        wide = torch.full((*dy.shape[:3], c.cout + 8), NAN, device=dev)
        wide[..., 4:4 + c.cout] = dy.to(dev)
        dyd = wide[..., 4:4 + c.cout]
    else:
        dyd = dy.to(dev)
    return src(x), src(x2), dyd


def _launch(layer, x, x2, dy, form, fill, dev):
    """One weight gradient in the given form; returns (dW in torch's layout, db, the guarded outputs or None)."""
    from interactive_spectrogram_inpainting.vqvae import _train
    with _fresh_memory_holds(fill):
        if form == "packed":
            dw, db = _train.conv_wgrad(layer, x, dy, x2=x2)
            return dw.contiguous(), db, None
        ow, ob = Out(tuple(layer.weight.shape), dev), Out(tuple(layer.bias.shape), dev)
        jobs = _train.ReduceJobs() if form == "deferred" else None
        dw, db = _train.conv_wgrad(layer, x, dy, x2=x2, out=(ow.view, ob.view), defer=jobs)
        assert dw is ow.view and db is ob.view
        if jobs is not None:
            assert jobs.jobs, "the deferred form returned no reduction job"
            jobs.flush()
        return dw, db, (ow, ob)


@pytest.mark.parametrize("c", TS.WGRAD_CASES, ids=TS.wgrad_case_id)
def test_weight_gradient_route(c, monkeypatch):
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.vqvae import _train
    from interactive_spectrogram_inpainting.vqvae.encoder_decoder import _ConvParams
    dev, L, case = _dev(), _hip.lib(), TS.wgrad_case_id(c)
    refs = TS.wgrad_case_refs(c)
    x, x2, dy = _device_operands(c, dev)
    layer = _ConvParams(c.c0 + c.c1, c.cout, c.k, c.stride, c.pad, transposed=c.transposed, groups=c.groups).to(dev)
    # the dispatcher's halo conditions, as the C-ABI reports them for the GEMM this launch is (roles swapped when transposed)
    if c.transposed:
        route_args = (c.c0, c.cout, 0, 4, 4, 2, 1, c.H, c.W)
    else:
        route_args = (c.cout, c.c0, c.c1, c.k, c.k, c.stride, c.pad, dy.shape[1], dy.shape[2])
    assert L.isi_conv_wgrad_halo_route(*route_args) == (1 if c.route == "halo" else 0)
    forms = ["packed"] if c.groups > 1 else ["torch", "deferred"] + ([] if c.layout == "pair" else ["packed"])
    by_flags = {}
    for flags in (2, 0, 4):
        monkeypatch.setattr(_train, "WGRAD_FLAGS", flags)
        if c.layout == "pair" and flags != 2:
            # pair-format sources are read by the halo-staged kernel alone, and that takes three-term products only
            with pytest.raises(_hip.HipLibraryError, match="pair-format"):
                _launch(layer, x, x2, dy, "torch", NAN, dev)
            continue
        dw, db, guards = _launch(layer, x, x2, dy, forms[0], NAN, dev)
        first = (dw.clone(), db.clone())
        if guards is not None:
            # a second launch into the same buffers: no accumulation, nothing stale
            with _fresh_memory_holds(NAN):
                _train.conv_wgrad(layer, x, dy, x2=x2, out=(guards[0].view, guards[1].view))
            assert guards[0].intact() and guards[1].intact(), f"{case} flags {flags}: a write outside dW or db"
        for form in forms:
            for fill in (0.0, NAN):
                dw2, db2, g2 = _launch(layer, x, x2, dy, form, fill, dev)
                assert _same_bits(dw2, first[0]) and _same_bits(db2, first[1]), \
                    f"{case} flags {flags}: the {form} form over memory holding {fill} differs from the first launch"
                assert g2 is None or (g2[0].intact() and g2[1].intact()), f"{case} flags {flags} {form}: a write outside dW or db"
        assert _same_bits(dw, first[0]) and _same_bits(db, first[1]), f"{case} flags {flags}: the second launch changed the values"
        by_flags[flags] = first
        mode = flags if c.vec else 0              # not vectorisable: the fp32 pipe whatever the flags
        if not c.vec and flags != 2:
            assert _same_bits(first[0], by_flags[2][0]), f"{case}: the scalar route depends on the precision flags"
            continue
        route = c.route if flags == 2 or not c.vec else {0: "f32-vector", 4: "six-term " + TS.wgrad_case_tile(c)}[flags]
        yard = TS.conv_wgrad_yardstick(mode, refs.spec_dw, refs.f32_dw, refs.model2, refs.model3)
        _check(case, route, flags, first[0], refs.spec_dw, yard, "dW")
        _check(case, route, flags, first[1], refs.spec_db, refs.f32_db, "db")


# ------------------------------------------------------------------------------------- the four-phase transposed C entry
@pytest.mark.parametrize("shape", TS.WGRAD_PHASE_CASES, ids=lambda s: "convT%dto%d-%dx%dx%d" % s[:5])
def test_four_phase_transposed_entry(shape):
    """isi_conv_wgrad_f32 with bit 0 of the flag word: blockIdx.z = phase * nsplit + split, phase (py, px) reads dY at
    dy_off = py * dst_sh + px * dst_sw and pads by (1 - py, 1 - px).  32 -> 64 is vectorisable (split kernel 128 x 128 under
    flags 2 / 4, conv_wgrad_f32_kernel under 0); 6 -> 8 has Cin % 4 != 0: scalar gather, fp32 pipe whatever the flags."""
    from interactive_spectrogram_inpainting import _hip
    cin, cout, B, H, W, vec = shape
    dev, L = _dev(), _hip.lib()
    case = "convT%dto%d-%dx%dx%d" % shape[:5]
    x, dy = TS.wgrad_phase_case_data(shape)
    a = (x, None, dy, 4, 2, 1, True)
    spec_dw, spec_db = TS.conv_wgrad_spec(*a)
    f32_dw, f32_db = TS.conv_wgrad_f32_yardstick(*a)
    m2, m3 = (TS.conv_wgrad_split_model(*a, pieces=2), TS.conv_wgrad_split_model(*a, pieces=3)) if vec else (None, None)
    xd = x.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    dyd = dy.to(dev)
    s0 = _hip.src_nchw_view(xd)
    K = 4 * cin
    Kpad = (K + 31) // 32 * 32
    nws = L.isi_conv_wgrad_workspace_floats(cout, K, B * H * W, 4)
    results = {}
    for flags in (2, 0, 4):
        runs = []
        for fill in (NAN, 0.0, NAN):
            dw, db, ws = Out((4, cout, Kpad), dev), Out((cout,), dev), Out((nws,), dev, fill=fill)
            rc = L.isi_conv_wgrad_f32(C.byref(s0), None, dyd.data_ptr(), dw.view.data_ptr(), db.view.data_ptr(), ws.view.data_ptr(),
                                      nws, B, H, W, cout, 4, 4, 2, 1, 1 | flags, None)
            assert rc == 0, L.isi_last_error()
            torch.cuda.synchronize()
            assert dw.intact() and db.intact() and ws.intact(), f"{case} flags {flags}: a write outside dW, db or the workspace"
            runs.append((dw.view.clone(), db.view.clone()))
        assert all(_same_bits(r[0], runs[0][0]) and _same_bits(r[1], runs[0][1]) for r in runs), \
            f"{case} flags {flags}: the result depends on what the workspace held"
        packed, db = runs[0]
        assert bool((packed[:, :, K:] == 0).all()), f"{case}: the padding columns K..Kpad of the packed gradient are not zero"
        results[flags] = packed
        if not vec and flags != 2:
            assert _same_bits(packed, results[2]), f"{case}: the scalar route depends on the precision flags"
            continue
        mode = flags if vec else 0
        route = "four-phase " + ({2: "split", 0: "f32-vector", 4: "six-term " + TS.wgrad_split_tile(cout, K)}[flags] if vec else "scalar")
        got = TS.convT_unpack_phases(packed.cpu(), cin, cout)
        _check(case, route, flags, got, spec_dw, TS.conv_wgrad_yardstick(mode, spec_dw, f32_dw, m2, m3), "dW")
        _check(case, route, flags, db, spec_db, f32_db, "db")


# --------------------------------------------------------------------------------------------------- isi_vq_embed_sum_f32
def _indices(kind, N, K, g):
    if kind == "uniform":
        return torch.randint(0, K, (N,), generator=g)
    if kind == "one code":
        return torch.full((N,), 3, dtype=torch.int64)
    if kind == "code 5 unused":
        i = torch.randint(0, K - 1, (N,), generator=g)
        return i + (i >= 5).long()
    assert kind == "last code"
    return torch.full((N,), K - 1, dtype=torch.int64)


@pytest.mark.parametrize("K", [32, 512])
@pytest.mark.parametrize("D", [4, 64, 128])
def test_embed_sum(D, K):
    """conv_wgrad_split_kernel<3, ..., ONEHOT>: D <= 64 runs the 64 x 256 tile, D = 128 the 128 x 128 one.  The kernel claims the
    exact float32 terms (three pieces of z against an operand exact in its hi piece), so its yardstick is the float32
    index_add.  Splits: min(256, 768 / tiles, nchunks / 8) -- N = 4099 is 129 chunks of 32 vectors, so 16 splits of 9 chunks
    (the last two of them short or empty) for every D and K here; N <= 33 is one split."""
    from interactive_spectrogram_inpainting import _hip
    dev, L = _dev(), _hip.lib()
    g = torch.Generator().manual_seed(D + K)
    for N in (1, 31, 33, 4099):
        z = torch.randn(N, D, generator=g)
        zd = z.to(dev)
        for kind in ("uniform", "one code", "code 5 unused", "last code"):
            idx = _indices(kind, N, K, g)
            case = f"embed_sum D={D} K={K} N={N} {kind}"
            nws = L.isi_vq_embed_sum_workspace_floats(D, K, N)
            out, ws = Out((D, K), dev), Out((nws,), dev)
            idx_d = idx.to(dev)
            rc = L.isi_vq_embed_sum_f32(zd.data_ptr(), idx_d.data_ptr(), out.view.data_ptr(), ws.view.data_ptr(), nws, N, D, K, None)
            assert rc == 0, L.isi_last_error()
            torch.cuda.synchronize()
            assert out.intact() and ws.intact(), f"{case}: a write outside the output or the workspace"
            got = out.view.cpu()
            unused = torch.ones(K, dtype=torch.bool)
            unused[idx] = False
            assert bool((got[:, unused] == 0.0).all()), f"{case}: the column of a code no vector chose is not exactly 0"
            _check(case, "one-hot", 4, got, TS.embed_sum_spec(z, idx, K), TS.embed_sum_f32(z, idx, K), "embed_sum")
            ws0 = Out((nws,), dev, fill=0.0)
            out2 = Out((D, K), dev)
            rc = L.isi_vq_embed_sum_f32(zd.data_ptr(), idx_d.data_ptr(), out2.view.data_ptr(), ws0.view.data_ptr(), nws, N, D, K, None)
            assert rc == 0 and _same_bits(out2.view.cpu(), got), f"{case}: the result depends on what the workspace held"


# --------------------------------------------------------------------------------------------------- isi_pad_channels4_f32
@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
def test_pad_channels4(Cc):
    from interactive_spectrogram_inpainting import _hip
    dev, L = _dev(), _hip.lib()
    B, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(Cc)
    base = torch.full((B, Cc + 1, H + 1, W + 3), NAN)
    base[:, 1:, :H, 1:W + 1] = torch.randn(B, Cc, H, W, generator=g)
    view = base.to(dev)[:, 1:, :H, 1:W + 1]                       # a non-contiguous NCHW view with NaN all around it
    assert not view.is_contiguous()
    out = Out((B, H, W, 4), dev)
    sv = _hip.src_nchw_view(view)
    assert L.isi_pad_channels4_f32(C.byref(sv), out.view.data_ptr(), B, H, W, None) == 0, L.isi_last_error()
    torch.cuda.synchronize()
    want = torch.nn.functional.pad(view.permute(0, 2, 3, 1), (0, 4 - Cc))
    assert out.intact() and _same_bits(out.view, want)
