"""The implicit-GEMM convolutions of csrc/conv_igemm_f32.hip against the float64 specification of tests/tests_support.py
(conv_spec), on every instance the dispatcher `launch_conv` selects: the three tile widths, the uniform, dual-source and
scalar-gather loaders, exact fp32 and the four split-product modes, pair-format sources and outputs, tap-major and
slice-major K order, narrow and wide tiles on both sides of the tile-count switch, every epilogue, the four-phase transposed
launch, and vqvae/_train.py conv_dgrad at the production channel counts.

Every case first asks the library which instance it runs (isi_conv2d_route / isi_conv_transpose2d_k4s2_route) and requires
the answer of the Python mirror tests_support.conv_route.  Every comparison is `tests_support.compare_rows`, per output
channel: the kernel may be 8 times as far from the float64 spec as the yardstick of the product mode it runs
(tests_support.conv_yardstick).  Outputs lie inside NaN buffers whose guards -- and, for a channel slice, the channels around
it -- must keep their bits; every launch runs once over NaN and once over zeros and the results must not differ by a bit.
tests/test_conv_igemm_host.py shows, without a GPU, what the comparison accepts and rejects.

A recording aid, not a check: with ISI_CONV_IGEMM_RECORD=<file> in the environment every comparison's error, yardstick and
ratio are written there when the module ends, with the module's wall time (profiles/conv_igemm_checks.txt is such a run)."""
import contextlib
import ctypes as C
import os
import time

import pytest
import torch

import tests_support as TS
from test_conv_wgrad_gpu import NAN, Out, _same_bits
from test_prior_gpu import _dev

pytestmark = pytest.mark.gpu

RECORD = []                    # (case, route, RowCheck)


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    t0 = time.time()
    yield
    path = os.environ.get("ISI_CONV_IGEMM_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# kernel error, yardstick of the mode (floored at 2^-23) and their ratio against the float64 spec, per comparison of\n"
                f"# tests/test_conv_igemm_gpu.py; metric and bound: tests_support.compare_rows (ratio <= {TS.ROW_OPS_MARGIN:g}).  Worst ratio first.\n"
                f"# wall time of the file, reference computations on the CPU included: {time.time() - t0:.1f} s\n")
        worst = {}
        for case, route, c in RECORD:
            worst[route] = max(worst.get(route, 0.0), c.ratio)
        for route in sorted(worst):
            f.write(f"# largest ratio, {route}: {worst[route]:.3f}\n")
        for case, route, c in sorted(RECORD, key=lambda r: -r[2].ratio):
            f.write(f"{c.ratio:8.3f}  err {c.err:.3e}  yardstick {c.yardstick:.3e}  {route}  {case} {c.what}\n")


def _check(case, route, got, spec, yardstick, what):
    got, spec, yardstick = TS.conv_rows(got), TS.conv_rows(spec), TS.conv_rows(yardstick)
    err, yard = TS.row_error(got, spec), max(TS.row_error(yardstick, spec), TS.ROW_OPS_FLOOR)
    print(f"{case} [{route}] {what}: err {err:.3e} yardstick {yard:.3e} ratio {err / yard:.3f}")
    RECORD.append((case, route, TS.RowCheck(what, err, yard, err / yard)))                  # (recorded whether it passes or not)
    TS.compare_rows(got, spec, yardstick, f"{case} [{route}] {what}")


def _nhwc_bits(t_nchw_view):
    """The storage-order (channels-last) contents of a [B, C, H, W] view, dense, on the CPU."""
    return t_nchw_view.permute(0, 2, 3, 1).contiguous().cpu()


class Operands:
    """The device tensors of a case: every source, the residual and the gate as [B, C, H, W] views, laid out by
    tests_support.conv_layout inside NaN storage (a read outside a view reaches the output as NaN); pair-format tensors hold
    the host encoding; the weight packed by the project's packers, with and without its split-f16 pair copy."""

    def __init__(self, c, dev):
        from interactive_spectrogram_inpainting.vqvae import _ops
        self.c, self.dev, self.data = c, dev, TS.conv_case_data(c)
        lay, d = TS.conv_layout(c), self.data
        self.store, self.view = {}, {}

        def put(name, values, pair=False):
            l = lay[name]
            s = torch.full((l.storage,), NAN, dtype=torch.float32, device=dev)
            v = s.as_strided(l.shape, l.strides, l.offset)
            if pair:
                assert v.permute(0, 2, 3, 1).is_contiguous(), "pair-format tensors are dense channels-last"
                values = TS.pair_encode_host(values.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
            v.copy_(values.to(dev))
            self.store[name], self.view[name] = s, v
        put("src0", d["x"], "0" in c.pairs)
        if c.c1:
            put("src1", d["x2"], "1" in c.pairs)
        if c.res:
            put("res", d["res"])
        if c.gate:
            lay["gate"] = lay["out"]
            put("gate", d["gate"], c.gate == "pair")
        # the fp32 tensors the pair-format sources were encoded from: what the mode-3 launch of a mode-4 case reads.  (Their
        # split is the pair's pieces bit for bit.  The DECODED value (hi + lo) / 4 would not do: where lo is exactly half
        # an ulp of an odd hi, it splits into (hi + ulp, -lo) -- the same value in other pieces, other roundings behind it.)
        self.fp32 = {}
        for name, key, flag in (("src0", "x", "0"), ("src1", "x2", "1")):
            if flag in c.pairs:
                self.fp32[name] = d[key].to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        w = d["w"].to(dev)
        pack = _ops.pack_convT_weight if c.op == "convT" else _ops.pack_conv_weight
        self.packed = {False: pack(w), True: pack(w, with_f16=True)}
        self.bias = d["bias"].to(dev) if c.bias else None

    def ptrs(self, out, with_f16):
        p = {name: s.data_ptr() for name, s in self.store.items()}
        p.update(out=out.view.data_ptr(), w=self.packed[with_f16].data_ptr())
        if self.bias is not None:
            p["bias"] = self.bias.data_ptr()
        return p


@contextlib.contextmanager
def _outputs_land_in(view_of_shape):
    """While active, torch.empty of exactly that shape returns the given tensor: the output vqvae/_ops.py allocates for a
    launch is the guarded buffer."""
    real, hits = torch.empty, [0]

    def placed(*a, **k):
        shape = tuple(a[0]) if len(a) == 1 and not isinstance(a[0], int) else tuple(a)
        if shape == tuple(view_of_shape.shape) and k.get("dtype", torch.float32) == torch.float32:
            hits[0] += 1
            return view_of_shape
        return real(*a, **k)
    torch.empty = placed
    try:
        yield
    finally:
        torch.empty = real
    assert hits[0] == 1, "the launch did not allocate its output through torch.empty"


def _launch(T, fill, mode=None, gate="case", pairs=None, fp32_sources=False):
    """One launch of the case (or of a variant: another precision, no gate, other pair formats, fp32 copies of the pair
    sources) into storage pre-filled with `fill`.  Returns (guarded storage, output as a [B, Cout, OH, OW] view, route)."""
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.vqvae import _ops
    c, L = T.c, _hip.lib()
    mode = c.mode if mode is None else mode
    pairs = c.pairs if pairs is None else pairs
    gate_kind = c.gate if gate == "case" else gate
    lay = TS.conv_layout(c)["out"]
    out = Out((lay.storage,), T.dev, fill=fill)
    view = out.view.as_strided(lay.shape, lay.strides, out.view.storage_offset() + lay.offset)   # (as_strided counts from the buffer's start)
    src = dict(T.view)
    if fp32_sources:
        src.update(T.fp32)
    x, x2, res = src["src0"], src.get("src1"), src.get("res")
    g = src["gate"].permute(0, 2, 3, 1) if gate_kind else None
    packed = T.packed[mode == 4]
    flags = TS.conv_case_flags(c, mode, gate, pairs)
    extra = flags & (32 | 64 | 128 | 512)
    ptrs = T.ptrs(out, mode == 4)
    ptrs.update({n: t.data_ptr() - 4 * TS.conv_layout(c)[n].offset for n, t in (("src0", x), ("src1", x2)) if t is not None})
    route = TS.conv_lib_route(L, c, ptrs, mode, gate, pairs)
    want = TS.conv_route(c, mode, gate, pairs)
    assert route == want, f"{TS.conv_case_id(c)}: the library runs {TS.conv_route_name(route)}, the mirror says {TS.conv_route_name(want)}"
    with contextlib.ExitStack() as stack:
        for name, value in c.knobs:
            stack.enter_context(_hip.knob(name, value))
        if c.op == "convT" and c.out in ("nhwc", "nchw"):
            target = view if c.out == "nchw" else view.permute(0, 2, 3, 1)
            with _outputs_land_in(target):
                y = _ops.conv_transpose2d_k4s2(x, packed, T.bias, c.cout, c.relu, out_nchw=c.out == "nchw", bf16x3=mode,
                                               extra_flags=extra, gate_nhwc=g)
        elif c.op == "conv" and c.out == "nhwc":
            with _outputs_land_in(view.permute(0, 2, 3, 1)):
                y = _ops.conv2d(x, packed, T.bias, c.cout, c.k, c.stride, c.pad, c.relu, x2_bchw=x2, residual_bchw=res, bf16x3=mode,
                                extra_flags=extra, gate_nhwc=g)
        else:                                             # an NCHW or sliced output: vqvae/_ops.py cannot express it
            s0, dst = _hip.src_nchw_view(x), _hip.dst_nchw_view(view)
            s1 = _hip.src_nchw_view(x2) if x2 is not None else None
            sr = _hip.src_nchw_view(res) if res is not None else None
            ref = lambda v: C.byref(v) if v is not None else None
            bias = T.bias.data_ptr() if T.bias is not None else None
            if c.op == "convT":
                a = (ref(dst), c.B, c.H, c.W, c.cout, flags, None)
                rc = (L.isi_conv_transpose2d_k4s2_gated_f32(ref(s0), packed.data_ptr(), bias, g.data_ptr(), *a) if g is not None else
                      L.isi_conv_transpose2d_k4s2_f32(ref(s0), packed.data_ptr(), bias, *a))
            else:
                a = (ref(dst), c.B, c.H, c.W, c.cout, c.k, c.k, c.stride, c.pad, flags, None)
                rc = (L.isi_conv2d_gated_f32(ref(s0), ref(s1), packed.data_ptr(), bias, ref(sr), g.data_ptr(), *a) if g is not None else
                      L.isi_conv2d_f32(ref(s0), ref(s1), packed.data_ptr(), bias, ref(sr), *a))
            assert rc == 0, L.isi_last_error()
            y = view
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device error: nothing that follows in this process could mean anything
        pytest.exit(f"{TS.conv_case_id(c)} [{TS.conv_route_name(route)}]: {e}", returncode=3)
    assert y.data_ptr() == view.data_ptr() and y.shape == view.shape and y.stride() == view.stride()
    what = f"{TS.conv_case_id(c)} over {fill}"
    assert out.intact(), f"{what}: a write outside the output's storage"
    if c.out == "slice":                                  # the channels around the slice keep what they held
        Cw = c.cout + 8
        wide = out.view.view(-1, Cw)
        around = torch.cat([wide[:, :4], wide[:, 4 + c.cout:]], dim=1)
        want_bits = torch.full_like(around, fill).view(torch.int32)
        assert torch.equal(around.view(torch.int32), want_bits), f"{what}: a write into the channels around the slice"
    return out, view, route


def _run(c, dev, **variant):
    """The NaN-filled and the zero-filled launch of a variant: equal in bits.  Returns (output view, route)."""
    T = variant.pop("T", None) or Operands(c, dev)
    (o1, v1, route), (o2, v2, _) = _launch(T, NAN, **variant), _launch(T, 0.0, **variant)
    assert _same_bits(_nhwc_bits(v1), _nhwc_bits(v2)), f"{TS.conv_case_id(c)}: the result depends on what the output held"
    return v1, route


SMALL = [c for c in TS.CONV_IGEMM_CASES if c not in set(TS.CONV_BIG_CASES)]


def _hold_case(c, dev):
    case = TS.conv_case_id(c)
    want = TS.conv_route(c)
    if want & 15 != 1:
        # a hand-off to a kernel with tests of its own: only the report is checked here
        from interactive_spectrogram_inpainting import _hip
        assert TS.conv_lib_route(_hip.lib(), c) == want and want > 0, case
        return
    T = Operands(c, dev)
    view, route = _run(c, dev, T=T)
    R = TS.conv_route_unpack(route)
    name = TS.conv_route_name(route)
    refs = TS.conv_case_refs(c)
    out_pair = "o" in c.pairs
    assert out_pair == bool(R.outp)
    if out_pair:
        got = TS.pair_decode_host(_nhwc_bits(view)).permute(0, 3, 1, 2)
    else:
        got = view.cpu()
    _check(case, name, got, refs.spec, TS.conv_refs_yardstick(refs, R.prec), "out")
    if c.mode and not R.prec:
        # a silent downgrade: the launch is held to the float32 yardstick above, and it is the exact launch bit for bit
        v0, r0 = _run(c, dev, T=T, mode=0)
        assert r0 == route and _same_bits(_nhwc_bits(v0), _nhwc_bits(view)), f"{case}: a split flag changed an exact-fp32 launch"
    if c.gate:
        plain, rp = _run(c, dev, T=T, gate=None)
        assert rp == route
        mask = TS.conv_gate_mask(T.data["gate"], c.gate == "pair").to(dev)
        assert 0.2 < float(mask.float().mean()) < 0.8
        want_bits = torch.where(mask, plain, torch.zeros_like(plain))
        assert _same_bits(_nhwc_bits(view), _nhwc_bits(want_bits)), f"{case}: the gated launch is not where(mask, plain launch, +0.0)"
    if out_pair:
        f32_out, rf = _run(c, dev, T=T, pairs=c.pairs.replace("o", ""))
        assert TS.conv_route_unpack(rf)._replace(outp=1) == R
        assert _same_bits(_nhwc_bits(view), TS.pair_encode_host(_nhwc_bits(f32_out))), \
            f"{case}: the pair-format output is not the encoding of the fp32 output of the same route"
    elif c.mode == 4 and R.prec >= 3:
        m3, r3 = _run(c, dev, T=T, mode=3, pairs="", fp32_sources=True)
        assert TS.conv_route_unpack(r3).prec == 3 and TS.conv_route_unpack(r3).bn == R.bn
        assert _same_bits(_nhwc_bits(m3), _nhwc_bits(view)), f"{case}: mode 4 (pack-time pieces, pair sources) differs from mode 3"


@pytest.mark.parametrize("c", SMALL, ids=TS.conv_case_id)
def test_convolution_route(c):
    _hold_case(c, _dev())


@pytest.mark.parametrize("c", TS.CONV_BIG_CASES, ids=TS.conv_case_id)
def test_narrow_wide_boundary(c):
    """tiles128 = 640 through the four phases (wide, every split mode, the pair-format output, a gate), 639 (narrow) and 642
    (wide, with residual, ReLU and gates of both formats) through three column tiles: the only large cases; their spec is
    computed once per shape and epilogue."""
    R = TS.conv_route_unpack(TS.conv_route(c))
    tiles128 = -(-c.B * c.H * c.W // TS.CONV_BM) * -(-c.cout // 128) * (4 if c.op == "convT" else 1)
    assert tiles128 in (639, 640, 642) and R.bn == (64 if tiles128 < 640 else 128) and R.prec == c.mode
    _hold_case(c, _dev())


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_loud_operands(poison, mode):
    """One inf / NaN in the source, with the ReLU: every output whose window holds it is NaN -- not 0, which fmaxf alone
    would make of it -- and every other output meets the spec."""
    dev = _dev()
    c = TS._cv(32, 72, 3, 1, 1, 2, 5, 7, mode=mode, relu=True)
    T = Operands(c, dev)
    b, ch, y, x = 1, 5, 2, 3
    T.view["src0"][b, ch, y, x] = poison
    (_, view, route) = _launch(T, NAN)
    assert TS.conv_route_unpack(route).prec == mode
    got = view.cpu()
    hit = torch.zeros(c.B, 1, c.H, c.W, dtype=torch.bool)
    hit[b, :, y - 1:y + 2, x - 1:x + 2] = True
    hit = hit.expand_as(got)
    assert bool(torch.isnan(got[hit]).all()), f"{int((~torch.isnan(got[hit])).sum())} outputs swallowed the {poison}"
    assert bool(torch.isfinite(got[~hit]).all())
    refs = TS.conv_case_refs(c)
    zero = lambda t: torch.where(hit, torch.zeros_like(t), t)
    _check(TS.conv_case_id(c) + f" {poison} in the source", TS.conv_route_name(route), zero(got), zero(refs.spec),
           zero(TS.conv_refs_yardstick(refs, mode)), "the other outputs")


# ------------------------------------------------------------------------------------------------ vqvae/_train.py conv_dgrad
DGRAD_LAYERS = {                # name: (cin, cout, k, stride, pad, transposed, residual)
    "conv3 128->128": (128, 128, 3, 1, 1, False, False), "res3 128->32": (128, 32, 3, 1, 1, False, True),
    "res1 32->128": (32, 128, 1, 1, 0, False, False), "k4s2 64->128": (64, 128, 4, 2, 1, False, False),
    "convT 128->64": (128, 64, 4, 2, 1, True, False), "quantize 192->64": (192, 64, 1, 1, 0, False, False),
    "quantize 64->64": (64, 64, 1, 1, 0, False, False),
}
_dgrad_model = []


def _production_model(dev):
    """A default VQ-VAE (128 hidden, 32 residual, 64 embedding channels) with its PackGroup refreshed: its layers' packed
    input-gradient weights come from the one batched pack launch."""
    if not _dgrad_model:
        from interactive_spectrogram_inpainting.vqvae import _train
        from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
        torch.manual_seed(11)
        m = VQVAE(in_channel=2).to(dev)
        m._dgrad_weights = _train._DgradWeights()
        grp = _train.PackGroup(m)
        grp.refresh()
        torch.cuda.synchronize()
        _dgrad_model.append((m, grp))
    return _dgrad_model[0][0]


def _dgrad_layer(dev, spec):
    """(layer, the _DgradWeights that serves it, owned by the model?)"""
    from interactive_spectrogram_inpainting.vqvae import _train
    from interactive_spectrogram_inpainting.vqvae.encoder_decoder import _ConvParams
    cin, cout, k, stride, pad, tr, _ = spec
    m = _production_model(dev)
    for layer in m.modules():
        if (isinstance(layer, _ConvParams) and (layer.in_channels, layer.out_channels, layer.kernel_size, layer.stride, layer.padding,
                                                layer.transposed, layer.groups) == (cin, cout, k, stride, pad, tr, 1)):
            return layer, m._dgrad_weights, True
    torch.manual_seed(cin * 7 + cout)
    return _ConvParams(cin, cout, k, stride, pad, transposed=tr).to(dev), _train._DgradWeights(), False


@pytest.mark.parametrize("precision", [None, 0], ids=["default", "bf16x3=0"])
@pytest.mark.parametrize("gate_kind", ["f32", "pair"])
@pytest.mark.parametrize("name", list(DGRAD_LAYERS))
def test_conv_dgrad_equals_float64_autograd(name, gate_kind, precision, monkeypatch):
    """The input gradient of a layer behind a ReLU (and, for the residual block's 3x3, inside a skip connection) against
    float64 autograd, at the production channel counts on a small ragged map; the weights once from a fresh _DgradWeights
    and, for the layers a model owns, once from its PackGroup: equal in bits."""
    from interactive_spectrogram_inpainting.vqvae import _ops, _train
    dev = _dev()
    spec = DGRAD_LAYERS[name]
    cin, cout, k, stride, pad, tr, with_res = spec
    layer, dw, owned = _dgrad_layer(dev, spec)
    fresh = _train._DgradWeights()
    if owned:
        assert id(layer) in dw.cache, "the PackGroup did not stamp this layer"
        assert _same_bits(dw.get(layer), fresh.get(layer)), f"{name}: the batched pack differs from the layer's own"
    if precision is not None:
        monkeypatch.setattr(_train, "DGRAD_PRECISION", precision)
    prec_asked = _train.DGRAD_PRECISION
    assert prec_asked == (1 if precision is None else 0)
    B, H, W = (2, 10, 22) if stride == 2 and not tr else (2, 9, 21)   # (k4 s2 p1 needs an even map for dX to have its shape: 5 x 11 phases)
    g = torch.Generator().manual_seed(len(name) * 31 + cin)
    w = layer.weight.detach().cpu()
    pre = torch.randn(B, cin, H, W, generator=g)
    a32 = torch.relu(pre)
    pre64 = pre.double().requires_grad_()
    a = torch.relu(pre64)
    if tr:
        y = torch.nn.functional.conv_transpose2d(a, w.double(), None, stride=2, padding=1)
    else:
        y = torch.nn.functional.conv2d(a, w.double(), None, stride=stride, padding=pad)
    dy = torch.randn(*y.shape, generator=g)
    skip = torch.randn(B, cin, H, W, generator=g) if with_res else None
    loss = (y * dy.double()).sum() + ((a * skip.double()).sum() if with_res else 0.0)
    loss.backward()
    want = pre64.grad
    # the same launch in the terms of the case table: its route, and the yardstick of the product mode it runs
    if tr:
        c = TS._cv(cout, cin, 4, 2, 1, B, y.shape[2], y.shape[3], mode=prec_asked, gate=gate_kind, bias=False)
        args = (dy, None, w, None, 4, 2, 1)
    elif stride == 2:
        c = TS._ct(cout, cin, B, y.shape[2], y.shape[3], mode=prec_asked, gate=gate_kind, bias=False)
        args = (dy, None, w, None, 4, 2, 1)
    else:
        c = TS._cv(cout, cin, k, 1, k - 1 - pad, B, y.shape[2], y.shape[3], mode=prec_asked, gate=gate_kind, bias=False,
                   res="nhwc" if with_res else None)
        args = (dy, None, w.flip(2, 3).transpose(0, 1).contiguous(), None, k, 1, k - 1 - pad)
    route = TS.conv_route(c)
    R = TS.conv_route_unpack(route)
    assert R.family == 1 and R.loader == 0 and R.prec == prec_asked, TS.conv_route_name(route)
    kw = dict(transposed=stride == 2 and not tr, res=skip, gate=a32, gate_pair=gate_kind == "pair")
    f32 = TS.conv_f32(*args, **kw)
    model = TS.conv_split_model(*args, mode=1, **kw) if R.prec else None
    spec64 = TS.conv_spec(*args, **kw)
    assert torch.allclose(spec64, want, rtol=1e-12, atol=1e-12)            # (the spec is that gradient: the host tests' identity)
    cl = lambda t: t.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    act = cl(a32)
    gate = _train.PairOnly(_ops.pair_encode(act)) if gate_kind == "pair" else act.permute(0, 2, 3, 1)
    # the route of the launch conv_dgrad really makes: the library is asked with the very arguments of its gated call (all
    # but the stream), in front of it
    from interactive_spectrogram_inpainting import _hip
    L, asked = _hip.lib(), []
    for entry, query in (("isi_conv2d_gated_f32", L.isi_conv2d_route),
                         ("isi_conv_transpose2d_k4s2_gated_f32", L.isi_conv_transpose2d_k4s2_route)):
        def spy(*a, _real=getattr(L, entry), _query=query):
            asked.append(_query(*a[:-1]))
            return _real(*a)
        monkeypatch.setattr(L, entry, spy)
    results = []
    for weights in ((dw, fresh) if owned else (fresh,)):
        got = _train.conv_dgrad(weights, layer, cl(dy), residual=cl(skip) if with_res else None, gate=gate)
        torch.cuda.synchronize()
        assert asked and asked[-1] == route, \
            f"{name}: conv_dgrad's launch runs {TS.conv_route_name(asked[-1]) if asked else 'no gated entry'}, the mirror says {TS.conv_route_name(route)}"
        assert got.shape == want.shape and got.permute(0, 2, 3, 1).is_contiguous()
        results.append(got.cpu())
    assert all(_same_bits(r, results[0]) for r in results)
    case = f"conv_dgrad {name} {B}x{H}x{W} gate {gate_kind} precision {prec_asked}"
    _check(case, TS.conv_route_name(route), results[0], want, TS.conv_yardstick(R.prec, want, f32, model), "dX")
    closed = ~(a32 > 0)
    assert bool((results[0][closed] == 0).all()) and not bool(torch.signbit(results[0][closed]).any()), f"{case}: a closed gate is not +0.0"
