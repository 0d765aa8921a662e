"""What tests/test_conv_igemm_gpu.py relies on, shown without a GPU: the float64 specification of the implicit-GEMM
convolutions (tests_support.conv_spec) against torch's float64 convolutions and their autograd input gradients, built the way
vqvae/_train.py conv_dgrad builds them; the Python mirror of the kernel route (tests_support.conv_route) against the library's
own answer (isi_conv2d_route / isi_conv_transpose2d_k4s2_route) at every case of the table and over a sweep; the case table
reaching everything on its list; the comparison accepting the float32 evaluation and every mode's own model at every small
case and rejecting every mutant on the list below; and the argument refusals of conv2d_batched_f32 /
conv_transpose2d_k4s2_f32 that return before anything touches a device (fake pointers)."""
import ctypes as C
import itertools

import pytest
import torch

import tests_support as TS

F = torch.nn.functional
BIG = set(TS.CONV_BIG_CASES)
SMALL = [c for c in TS.CONV_IGEMM_CASES if c not in BIG]
IGEMM = [c for c in SMALL if TS.conv_route(c) > 0 and TS.conv_route(c) & 15 == 1]


def _find(**want):
    """The first small igemm case with these fields."""
    for c in IGEMM:
        if all(getattr(c, k) == v for k, v in want.items()):
            return c
    raise AssertionError(f"no case with {want}")


# ------------------------------------------------------------------------------------------------------------ the spec
def _r64(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("two,stride,pad,k", [(False, 1, 1, 3), (True, 1, 0, 3), (False, 1, 2, 3), (False, 2, 1, 4), (True, 1, 0, 1)])
def test_conv_spec_equals_torch_float64(two, stride, pad, k):
    g = torch.Generator().manual_seed(k * 10 + pad)
    x, x2 = _r64(g, 2, 5, 7, 9), (_r64(g, 2, 3, 7, 9) if two else None)
    w, b = _r64(g, 6, 8 if two else 5, k, k), _r64(g, 6)
    want = F.conv2d(torch.cat([x, x2], 1) if two else x, w, b, stride=stride, padding=pad)
    res, gate = _r64(g, *want.shape), TS.gate_data(want.numel(), g)[1].reshape(want.shape)
    assert torch.allclose(TS.conv_spec(x, x2, w, b, k, stride, pad), want, rtol=1e-13, atol=1e-13)
    full = torch.relu(want + res) * (gate > 0)
    assert torch.allclose(TS.conv_spec(x, x2, w, b, k, stride, pad, res=res, relu=True, gate=gate), full, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (2, 2)])
def test_transposed_spec_equals_torch_float64(H, W):
    g = torch.Generator().manual_seed(H * 10 + W)
    x, w, b = _r64(g, 2, 5, H, W), _r64(g, 5, 6, 4, 4), _r64(g, 6)
    want = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    assert torch.allclose(TS.conv_spec(x, None, w, b, 4, 2, 1, transposed=True), want, rtol=1e-13, atol=1e-13)
    gate = TS.gate_data(want.numel(), g)[1].reshape(want.shape)
    assert torch.allclose(TS.conv_spec(x, None, w, b, 4, 2, 1, transposed=True, relu=True, gate=gate), torch.relu(want) * (gate > 0),
                          rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("kind", ["k3p1", "k3p0", "k1", "k4s2", "transposed"])
def test_input_gradients_equal_float64_autograd(kind):
    """The input gradient of a layer fed by a ReLU, with a skip connection around the layer, as vqvae/_train.py conv_dgrad
    launches it: the convolution of dY (k3 / k1 layers: the flipped, transposed weight with pad k - 1 - p; k4 s2 layers: the
    transposed form with the same weight tensor; transposed layers: the strided form with the same weight tensor), the skip
    gradient as the residual, the rectified activation the layer consumed as the gate."""
    g = torch.Generator().manual_seed(len(kind))
    pre = _r64(g, 2, 5, 6, 8).requires_grad_()
    a = torch.relu(pre)
    if kind == "transposed":
        w = _r64(g, 5, 4, 4, 4)
        y = F.conv_transpose2d(a, w, None, stride=2, padding=1)
    else:
        k, s, p = {"k3p1": (3, 1, 1), "k3p0": (3, 1, 0), "k1": (1, 1, 0), "k4s2": (4, 2, 1)}[kind]
        w = _r64(g, 4, 5, k, k)
        y = F.conv2d(a, w, None, stride=s, padding=p)
    dy, skip = _r64(g, *y.shape), _r64(g, *a.shape)
    ((y * dy).sum() + (a * skip).sum()).backward()
    gate = a.detach()
    if kind == "transposed":
        got = TS.conv_spec(dy, None, w, None, 4, 2, 1, res=skip, gate=gate)
    elif kind == "k4s2":
        got = TS.conv_spec(dy, None, w, None, 4, 2, 1, transposed=True, gate=gate) + skip * (gate > 0)   # (no residual input there)
    else:
        got = TS.conv_spec(dy, None, w.flip(2, 3).transpose(0, 1), None, k, 1, k - 1 - p, res=skip, gate=gate)
    assert torch.allclose(got, pre.grad, rtol=1e-13, atol=1e-13)


def test_pair_format_operands_and_gates_of_the_spec():
    """A pair-format source is what its pairs decode to; a pair-format gate is closed where the decoded activation is not
    positive -- below 2^-26 the hi piece f16(4 x) is zero -- while the fp32 gate lets those through."""
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(1, 8, 3, 4, generator=g), torch.randn(8, 8, 1, 1, generator=g)
    xr = TS.pair_round_f16(x)
    assert not torch.equal(xr, x)
    assert torch.equal(TS.conv_spec(x, None, w, None, 1, 1, 0, pair0=True), TS.conv_spec(xr, None, w, None, 1, 1, 0))
    gate = torch.tensor([1.0, 2.0 ** -26, 2.0 ** -27, 2.0 ** -30, 0.0, -0.0, -1.0, 6e-8]).reshape(1, 8, 1, 1)
    assert TS.conv_gate_mask(gate).reshape(-1).tolist() == [True, True, True, True, False, False, False, True]
    assert TS.conv_gate_mask(gate, gate_pair=True).reshape(-1).tolist() == [True, True, False, False, False, False, False, True]
    d = TS.conv_case_data(_find(gate="pair"))["gate"]
    f32, pair = TS.conv_gate_mask(d), TS.conv_gate_mask(d, gate_pair=True)
    assert bool((f32 & ~pair).any()) and not bool((pair & ~f32).any()) and 0.3 < float(f32.float().mean()) < 0.7
    assert bool(((d == 0) & torch.signbit(d)).any())                          # -0.0 among the zeros


# ------------------------------------------------------------------------------------------------------------ the route
def test_case_table_reaches_everything_on_its_list():
    assert TS.conv_igemm_coverage_gaps(TS.CONV_IGEMM_CASES) == []
    ids = [TS.conv_case_id(c) for c in TS.CONV_IGEMM_CASES]
    assert len(set(ids)) == len(ids)
    # the list is a check: without the large cases, or without the dual-source ones, it is not empty
    assert "four-phase: tiles128 640" in TS.conv_igemm_coverage_gaps(SMALL)
    assert TS.conv_igemm_coverage_gaps([c for c in TS.CONV_IGEMM_CASES if not (c.c1 and c.c0 % 32)])


def _variants(c):
    """The launches the GPU test makes of a case: (mode, gate, pairs)."""
    v = [(None, "case", None)]
    if c.gate:
        v.append((None, None, None))
    if c.mode == 4:
        v.append((3, "case", ""))
    if "o" in c.pairs:
        v.append((None, "case", c.pairs.replace("o", "")))
    return v


def test_library_route_equals_the_mirror_at_every_case():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    for c in TS.CONV_IGEMM_CASES:
        for mode, gate, pairs in _variants(c):
            got, want = TS.conv_lib_route(L, c, None, mode, gate, pairs), TS.conv_route(c, mode, gate, pairs)
            assert got == want, f"{TS.conv_case_id(c)} {(mode, gate, pairs)}: library {TS.conv_route_name(got)}, mirror {TS.conv_route_name(want)}"
    # what the routes pin: mode 3 below K = 128 and every split flag on a dual-source / gather launch run the exact instance;
    # mode 4 at Cout <= 32 runs PREC 3
    r = TS.conv_route_unpack(TS.conv_lib_route(L, _find(c0=96, mode=3)))
    assert (r.bn, r.loader, r.prec) == (64, 0, 0)
    for c in IGEMM:
        r = TS.conv_route_unpack(TS.conv_lib_route(L, c))
        assert r.prec == 0 or r.loader == 0, TS.conv_case_id(c)
        if c.mode == 4 and c.cout <= 32 and r.loader == 0:
            assert r.prec == 3


def test_library_route_equals_the_mirror_over_a_sweep():
    """Cout, K, M, flags, layouts, gates, pair formats and knobs, refusals included (the statuses must agree too)."""
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    n = routes = 0
    seen = set()

    def check(c, **kw):
        nonlocal n
        got, want = TS.conv_lib_route(L, c, **kw), TS.conv_route(c, **kw)
        assert got == want, f"{c} {kw}: library {TS.conv_route_name(got)}, mirror {TS.conv_route_name(want)}"
        seen.add(got)
        n += 1
    pair_sets = ("", "0", "1", "01", "o", "0o", "01o")
    for c0, c1, k, stride, pad in ((2, 0, 4, 2, 1), (4, 0, 3, 1, 1), (3, 0, 3, 1, 1), (16, 0, 1, 1, 0), (32, 0, 1, 1, 0), (64, 0, 1, 1, 0),
                                   (96, 0, 1, 1, 0), (128, 0, 1, 1, 0), (256, 0, 1, 1, 0), (32, 0, 3, 1, 1), (32, 32, 3, 1, 1),
                                   (36, 28, 3, 1, 1), (32, 64, 1, 1, 0), (64, 0, 4, 2, 1), (16, 0, 4, 2, 1)):
        for cout in (1, 32, 33, 64, 65, 72, 128, 129):
            for B, H, W in ((1, 1, 300), (2, 5, 7), (1, 16, 16)):
                for mode in range(5):                       # (a one-row map under k4 s2 p1 has no output: refused, -1)
                    for pairs in (pair_sets if mode >= 3 else ("", "0")):
                        if "1" in pairs and not c1:
                            continue
                        for gate, res in ((None, None), ("f32", None), ("pair", "nhwc"), (None, "nchw")):
                            check(TS._cv(c0, cout, k, stride, pad, B, H, W, mode=mode, c1=c1, pairs=pairs, gate=gate, res=res))
                for src0, out in (("nchw", "nhwc"), ("off1", "nhwc"), ("row", "slice"), ("slice", "nchw")):
                    for mode in (0, 1, 4):
                        check(TS._cv(c0, cout, k, stride, pad, B, H, W, mode=mode, c1=c1, src0=src0, out=out))
                for knob in ("ISI_NO_CONV_PAIR_KERNEL", "ISI_CONV_PAIR_ALL", "ISI_NO_CONV_FIRST", "ISI_NO_GEMM_KERNEL"):
                    for mode, pairs in ((1, ""), (4, "0o" if not c1 else "01o")):
                        check(TS._cv(c0, cout, k, stride, pad, B, H, W, mode=mode, c1=c1, pairs=pairs, knobs=((knob, 1),)))
    for cin in (6, 16, 32, 48, 64):
        for cout in (1, 2, 4, 5, 64, 72, 96, 128):
            for B, H, W in ((1, 1, 1), (2, 3, 5)):
                for mode in range(5):
                    for pairs in (("", "0", "o", "0o") if mode >= 3 else ("", "0")):
                        for gate in (None, "f32", "pair"):
                            for knobs in ((), (("ISI_NO_CONVT_PAIR_KERNEL", 1),)):
                                check(TS._ct(cin, cout, B, H, W, mode=mode, pairs=pairs, gate=gate, knobs=knobs))
                    for src0, out in (("nchw", "nhwc"), ("nhwc", "nchw"), ("slice", "slice")):
                        check(TS._ct(cin, cout, B, H, W, mode=mode, src0=src0, out=out))
    # the narrow / wide line: tiles128 = 636 | 640 through the four phases, 639 | 642 through three column tiles, both sides
    # in every split mode; beside it the widths that never switch
    for mode in range(5):
        for W, bn in ((160, 64), (161, 128)):
            c = TS._ct(32, 96, 1, 127, W, mode=mode)
            check(c)
            assert TS.conv_route_unpack(TS.conv_route(c)).bn == (bn if mode else 128)
        for H, W, bn in ((142, 192, 64), (143, 191, 128)):
            c = TS._cv(128, 264, 1, 1, 0, 1, H, W, mode=mode)
            check(c)
            assert TS.conv_route_unpack(TS.conv_route(c)).bn == (bn if mode else 128)
        check(TS._cv(128, 64, 1, 1, 0, 1, 640, 128, mode=mode))
        check(TS._cv(128, 65, 1, 1, 0, 1, 640, 128, mode=mode))
    assert n > 5000 and len(seen) > 40, (n, len(seen))
    assert {TS.CONV_E_UNSUPPORTED} | set(range(2, 8)) <= {s if s < 0 else s & 15 for s in seen}     # every hand-off, and refusals


# ------------------------------------------------------------------------------------------------------ the comparison
@pytest.mark.parametrize("c", IGEMM, ids=TS.conv_case_id)
def test_float32_evaluation_and_the_models_pass_the_comparison(c):
    """Under the yardstick of every mode: the float32 evaluation (modes 0, 1, 3 / 4: it is half of their yardstick) and the
    mode's own model (modes 1, 2, 3 / 4)."""
    refs = TS.conv_case_refs(c, modes=(1, 2, 3))
    what = TS.conv_case_id(c)
    for prec in (0, 1, 3):
        TS.conv_hold(refs.f32, refs, prec, f"{what} float32 as prec {prec}")
    for prec in (1, 2, 3):
        chk = TS.conv_hold(refs.models[prec], refs, prec, f"{what} model {prec}")
        assert chk.ratio <= 1.0 + 1e-9


def _rejected(got, refs, prec, what):
    with pytest.raises(AssertionError, match="times the float32 yardstick"):
        TS.conv_hold(got, refs, prec, what)


def _mutant(c, **mutant):
    d = TS.conv_case_data(c)
    a, kw = TS.conv_case_args(c, d)
    return TS.conv_f32(*a, **kw, **mutant)


MUTANTS = [
    ("the last K chunk dropped, K = 36", dict(c0=4, cout=1), dict(drop_last_chunk=True)),
    ("the last K chunk dropped, K = 100", dict(c0=100, mode=1), dict(drop_last_chunk=True)),
    ("the last K chunk dropped, K = 124", dict(c0=124), dict(drop_last_chunk=True)),
    ("padding off by one on one side", dict(c0=32, cout=40, k=3, pad=1, B=1, H=31, mode=0), dict(pad_shift=True)),
    ("padding off by one on one side, pad 2", dict(c0=32, cout=40, k=3, pad=2, mode=1), dict(pad_shift=True)),
    ("one border tap missing", dict(c0=32, cout=40, k=3, pad=1, B=3, mode=1), dict(border_tap=True)),
    ("one border tap missing, stride 2", dict(c0=32, cout=40, k=4, stride=2, H=9), dict(border_tap=True)),
    ("the two sources swapped", dict(c0=36, c1=28, mode=0, relu=False), dict(swap_sources=True)),
    ("the two sources swapped, 32 + 64", dict(c0=32, c1=64, mode=0), dict(swap_sources=True)),
    ("the batch seam ignored", dict(c0=32, cout=40, B=3, mode=0), dict(seam_tile=TS.CONV_BM)),
    ("the bias missing in the last column tile", dict(c0=4, cout=130), dict(bias_tile=128)),
    ("the bias missing in the last 32 columns' wave", dict(c0=8, cout=33, src0="nhwc"), dict(bias_tile=32)),
    ("the residual added after the ReLU", dict(res="nhwc", relu=True, cout=72, mode=1), dict(res_after_relu=True)),
    ("gate >= instead of >", dict(gate="f32", res="nchw", cout=64, mode=0), dict(gate_ge=True)),
    ("gate >= instead of >, four phases", dict(op="convT", gate="f32", c0=32), dict(gate_ge=True)),
    ("a pair-format gate read from the wrong half-word", dict(gate="pair", cout=72, mode=1), dict(gate_wrong_half=True)),
    ("a pair-format gate read from the wrong half-word, four phases", dict(op="convT", gate="pair", c0=48), dict(gate_wrong_half=True)),
    ("the phases (py, px) exchanged", dict(op="convT", c0=32, cout=96, B=2, mode=0), dict(swap_phases=True)),
    ("the phases (py, px) exchanged, NCHW output", dict(op="convT", out="nchw", mode=1), dict(swap_phases=True)),
]


@pytest.mark.parametrize("name,want,mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_comparison_rejects_the_mutant(name, want, mutant):
    c = _find(**want)
    refs = TS.conv_case_refs(c, modes=(1, 3))
    got = _mutant(c, **mutant)
    assert got.shape == refs.spec.shape
    for prec in (0, 1, 3):                               # under the loosest yardstick too
        _rejected(got, refs, prec, name)
    TS.conv_hold(_mutant(c), refs, 0, name + ": the unmutated evaluation")


@pytest.mark.parametrize("want", [dict(c0=32, cout=32, k=3, mode=1), dict(c0=32, cout=72, k=3, mode=1, res=None, gate=None, relu=False),
                                  dict(c0=64, cout=192, mode=1), dict(op="convT", c0=32, cout=96, B=2, mode=1)],
                         ids=["128x32", "narrow", "K=64", "four-phase"])
def test_comparison_rejects_wrong_term_counts(want):
    """A two-term product in modes 1 and 3 (either cross term left out), and a three-term product -- bf16 or f16 pieces --
    passed off as mode 2."""
    c = _find(**want)
    refs = TS.conv_case_refs(c, modes=(1, 2, 3))
    a, kw = TS.conv_case_args(c, TS.conv_case_data(c))
    for mode in (1, 3):
        for drop in ("hi_lo", "lo_hi"):
            _rejected(TS.conv_split_model(*a, mode=mode, drop=drop, **kw), refs, mode, f"mode {mode} without {drop}")
    _rejected(refs.models[1], refs, 2, "three bf16 terms as mode 2")
    xc = TS._conv_cat(*a[:2], torch.float32)
    rows, W2d, _ = TS._conv_gemms(xc, a[2], *a[4:], c.op == "convT")[0]
    r2 = rows.reshape(-1, rows.shape[-1])
    full, part = TS.conv_six_term_product(r2, W2d), TS.conv_six_term_product(r2, W2d, drop_mid=True)
    exact = r2.double() @ W2d.double().t()
    assert TS.row_error(full.t(), exact.t()) < 2.0 ** -23 < 2.0 ** -19 < TS.row_error(part.t(), exact.t())


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_before_anything_touches_a_device():
    """Every call below returns from conv2d_batched_f32 / conv_transpose2d_k4s2_f32 / launch_conv (csrc/conv_igemm_f32.hip)
    through `invalid` / `unsupported` ahead of the first HIP call of its path -- the checks sit in front of
    hipFuncSetAttribute and the launch in launch_cfg, and no `zero` words are passed, so vq_zero_counts is not reached.  The
    pointers are fake: a path that touched them would crash this process."""
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    fake = TS.CONV_FAKE_PTR
    ref = lambda v: C.byref(v) if v is not None else None

    def conv(c, flags, w=fake, gate=None, res="case", twin=None):
        s0, s1, r, dst = TS.conv_lib_views(c)
        r = r if res == "case" else res
        a = (c.B, c.H, c.W, c.cout, c.k, c.k, c.stride, c.pad, flags, None)
        if twin:
            return L.isi_conv2d_twin_f32(ref(s0), ref(s1), w, None, ref(dst), twin, *a)
        if gate:
            return L.isi_conv2d_gated_f32(ref(s0), ref(s1), w, None, ref(r), gate, ref(dst), *a)
        return L.isi_conv2d_f32(ref(s0), ref(s1), w, None, ref(r), ref(dst), *a)

    def convT(c, flags, w=fake, gate=None, twin=None):
        s0, _, _, dst = TS.conv_lib_views(c)
        a = (c.B, c.H, c.W, c.cout, flags, None)
        if twin:
            return L.isi_conv_transpose2d_k4s2_twin_f32(ref(s0), w, None, ref(dst), twin, *a)
        if gate:
            return L.isi_conv_transpose2d_k4s2_gated_f32(ref(s0), w, None, gate, ref(dst), *a)
        return L.isi_conv_transpose2d_k4s2_f32(ref(s0), w, None, ref(dst), *a)

    def refused(rc, status, text):
        assert rc == status and text in L.isi_last_error().decode(), (rc, L.isi_last_error())
    c = TS._cv(32, 72, 3, 1, 1, 2, 5, 7)
    t = TS._ct(32, 72, 2, 3, 5)
    f16 = 8 | 16
    # pair formats outside the split-f16 kernels: exact fp32, three bf16 terms, no pack-time pieces, Cout <= 32, K < 128, gather
    for flags in (32, 128, 2 | 32, 8 | 32, 4 | 128):
        refused(conv(c, flags), -4, "pair-format tensors need the split-f16 kernels")
        refused(convT(t, flags), -4, "pair-format tensors need the split-f16 kernels")
    refused(conv(c._replace(cout=32), f16 | 32), -4, "pair-format tensors need")
    refused(conv(TS._cv(32, 72, 1, 1, 0, 2, 5, 7), f16 | 32), -4, "pair-format tensors need")
    refused(conv(c._replace(src0="nchw"), f16 | 32), -4, "pair-format tensors need")
    refused(conv(c._replace(out="nchw"), f16 | 128), -4, "pair-format output is channels-last")
    refused(conv(c._replace(cout=68), f16 | 128), -4, "Cout % 8 == 0")
    # a twin without the LDS-DMA kernel: Cout % 64 != 0; the kernel switched off
    refused(conv(c, f16 | 32 | 128, twin=fake), -4, "written by the LDS-DMA kernel only")
    with _hip.knob("ISI_NO_CONV_PAIR_KERNEL", 1):
        refused(conv(c._replace(cout=64), f16 | 32 | 128, twin=fake), -4, "written by the LDS-DMA kernel only")
    refused(conv(c._replace(cout=64), f16 | 32, twin=fake), -4, "an fp32 twin accompanies")
    refused(convT(t, f16 | 32 | 128, twin=fake), -4, "written by the fused pair kernel only")
    refused(convT(t, f16 | 128, twin=fake), -4, "an fp32 twin accompanies")
    # a residual with pair formats; a gate with pair-format sources or output
    refused(conv(c._replace(res="nhwc"), f16 | 32), -4, "pair formats with a residual input")
    refused(conv(c._replace(res="nhwc"), f16 | 128), -4, "pair formats with a residual input")
    for flags in (f16 | 32, f16 | 128, f16 | 64):
        refused(conv(c, flags, gate=fake), -4, "gated epilogue")
    for flags in (f16 | 32, f16 | 128):
        refused(convT(t, flags, gate=fake), -4, "gated epilogue")
    refused(convT(TS._ct(32, 2, 2, 3, 5), 0, gate=fake), -4, "gated epilogue")                      # the few-channel kernel has none
    # an unaligned packed weight
    refused(conv(c, 0, w=fake + 4), -1, "16-byte aligned")
    refused(convT(t, 0, w=fake + 4), -1, "16-byte aligned")
    # a tensor of 4 GiB (2^30 floats): source, output, residual
    big = TS._cv(4, 4, 3, 1, 1, 1, 16384, 16384)
    assert TS._extent(TS.conv_layout(big)["src0"]) == 1 << 30
    refused(conv(big, 0), -4, "4 GiB")
    refused(conv(TS._cv(4, 16, 1, 1, 0, 1, 8192, 8192), 0), -4, "4 GiB")                           # the output alone
    refused(conv(TS._cv(4, 12, 1, 1, 0, 1, 8192, 8192, out="nhwc", res="slice"), 0), -4, "4 GiB")  # the residual alone
    refused(convT(TS._ct(4, 4, 1, 8192, 8192), 0), -4, "4 GiB")
    assert conv(TS._cv(4, 4, 3, 1, 1, 1, 16384, 16383), 0, w=fake + 4) == -1                       # just below: past that check
    # and the route queries give the same answers
    assert TS.conv_lib_route(L, c._replace(mode=4, pairs="0", res="nhwc")) == -4
    assert TS.conv_lib_route(L, big) == -4
