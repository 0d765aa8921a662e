"""The fused quantize_conv + codebook search (vq_conv1x1_nearest_kernel of csrc/vq_nearest.hip) against the float64
specification of tests/tests_support.py (vq_fused_spec), at its own entry points isi_vq_conv1x1_nearest_f32 and
isi_vq_conv1x1_nearest_tape_f32, through ctypes with explicit isi_src strides: every chunk-count template (NCH 2, 4, 6, 8,
with and without a dead chunk), a second source on an even and on an odd chunk, cropped channel slices of wider maps,
pixel counts from 1 to 66 603 (a second grid-stride pass and a ragged last tile), codebooks of 16 codes to the largest the
launch accepts, duplicate codes, far codes, non-finite codes and activations, and the refusals.

The case data (tests_support.vq_fused_case_data) has no near-tie -- the float64 gap between the best and the second-best
code is at least 1e-4 of |z|^2 + |e|^2, three decades above where a float32 evaluation flips an index -- so every index
must equal the spec's.  Per case: idx and the histogram exactly (the tape entry starts from garbage counts); z of the tape
entry through `compare_rows` against the worse of the float32 evaluation and the three-term split-f16 model (margin 8,
floor 2^-23); q within one float32 ulp of max(|z|, |e|) of e_idx and bit-identical between the entries; the pair copy within
2^-23 max|q| of q and the same bits without q_out; every partial of the squared error written and their sum within 1e-5 of
the spec's; isi_vq_finalize_f32 on top of them; for dense sources the header's promise -- isi_conv2d_f32(ISI_CONV_F16X3 |
ISI_CONV_W16) followed by isi_vq_nearest_flags_f32(ISI_CONV_F16X3) gives the same bits (from 128 input channels on, where
that convolution runs split products; below, the same idx and counts); and the workspace holds what
isi_vq_pack_fragments_f32 makes of the same weight.  Every output lies in a buffer of NaN (integers: a sentinel) whose
guards must keep their bits, every input must be unchanged, and a strided source lies in a parent map that is NaN outside
the view: a read outside it shows up as index -1.  tests/test_vq_fused_host.py shows, without a GPU, what the comparisons
reject.

A recording aid, not a check: with ISI_VQ_FUSED_RECORD=<file> in the environment every comparison's error, yardstick and
ratio are written there when the module ends, the worst ratio first (profiles/vq_fused_checks.txt is such a run on an
MI355X: the worst ratio there is 2.51, z of the single pixel of N = 1 at (64, 128) channels; from 31 pixels on z stays below
1.5, and diff and perplexity below 1)."""
import ctypes as C
import os

import pytest
import torch

import tests_support as TS
from test_prior_gpu import _dev

pytestmark = pytest.mark.gpu

PAD = 64                       # elements in front of and behind every buffer (16-byte alignment stays)
D = TS.VQ_FUSED_D
NAN = float("nan")
SENTINEL = -7777               # idx before a launch (no NaN among integers)
COUNT_GUARD = 2 ** 30
RECORD = []                    # RowCheck of every comparison of this process
ROUTE = TS.VQ_FUSED_ROUTE_CASES[6]                        # (64, 128), K = 512, N = 257
assert (ROUTE.C0, ROUTE.C1, ROUTE.K) == (64, 128, 512)


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_VQ_FUSED_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# kernel error, yardstick (floored at 2^-23) and their ratio against the float64 spec, per comparison of\n"
                f"# tests/test_vq_fused_gpu.py; metric and bound: tests_support.compare_rows (ratio <= {TS.ROW_OPS_MARGIN:g}).  Worst ratio first.\n")
        for c in sorted(RECORD, key=lambda r: -r.ratio):
            f.write(f"{c.ratio:8.3f}  err {c.err:.3e}  yardstick {c.yardstick:.3e}  {c.what}\n")


def _lib():
    from interactive_spectrogram_inpainting import _hip
    return _hip, _hip.lib(), _dev()


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))


class Buf:
    """n elements inside a flat buffer of `fill`, PAD elements in front and behind; `src` fills the view."""

    def __init__(self, n, dev, fill=NAN, dtype=torch.float32, src=None):
        self.buf = torch.full((PAD + n + PAD,), fill, dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + n]
        if src is not None:
            self.view.copy_(src.reshape(-1))
        self.before = self.buf.clone()
        self.ptr = self.view.data_ptr()

    def intact(self):
        """The guards keep their bits."""
        return _same(self.buf[:PAD], self.before[:PAD]) and _same(self.buf[-PAD:], self.before[-PAD:])

    def untouched(self):
        return _same(self.buf, self.before)

    def cpu(self, *shape):
        return self.view.cpu().reshape(*shape) if shape else self.view.cpu()


class Source:
    """One source of the launch in the pair format.  Dense: [B, H, W, C].  Strided (`parent` = one of VQ_FUSED_PARENTS): a
    channel slice of a wider map, cropped in H and W, everything outside the view NaN before the encoding -- so the pieces
    there decode to NaN, which is checked -- and the whole in NaN guards."""

    def __init__(self, _hip, L, a, B, H, W, dev, parent=None):
        Cc = a.shape[1]
        extra, c0, top, bottom, left, right = parent if parent is not None else (0, 0, 0, 0, 0, 0)
        Cp, Hp, Wp = Cc + extra, H + top + bottom, W + left + right
        full = torch.full((B, Hp, Wp, Cp), NAN)
        inside = torch.zeros((B, Hp, Wp, Cp), dtype=torch.bool)
        full[:, top:top + H, left:left + W, c0:c0 + Cc] = a.reshape(B, H, W, Cc)
        inside[:, top:top + H, left:left + W, c0:c0 + Cc] = True
        n = full.numel()
        plain = Buf(n, dev, src=full)
        self.enc = Buf(n, dev)
        assert L.isi_pair_encode_f32(plain.buf.data_ptr(), self.enc.buf.data_ptr(), plain.buf.numel(), None) == 0, L.isi_last_error()
        dec = torch.empty_like(plain.buf)
        assert L.isi_pair_decode_f32(self.enc.buf.data_ptr(), dec.data_ptr(), dec.numel(), None) == 0, L.isi_last_error()
        torch.cuda.synchronize()
        self.enc.before = self.enc.buf.clone()
        dec_in = dec[PAD:PAD + n].cpu().reshape(B, Hp, Wp, Cp)
        keep = inside & torch.isfinite(full) & (full.abs() < TS.VQ_FUSED_ACT_LIMIT)      # (a test's loud activations are poison too)
        assert TS.same_bits(dec_in[keep], full[keep]), "the pair format holds the activations exactly"
        assert not bool(torch.isfinite(dec_in[~keep]).any()) and not bool(torch.isfinite(dec[:PAD]).any()) \
            and not bool(torch.isfinite(dec[-PAD:]).any()), "the poison outside the view decodes non-finite"
        first = (top * Wp + left) * Cp + c0
        self.strides = (Hp * Wp * Cp, 1, Wp * Cp, Cp)
        self.src = _hip.isi_src(self.enc.ptr + 4 * first, Cc, *self.strides)
        self.offset = first
        self.dense_f32 = None if parent is not None else plain     # the fp32 map, for the two-launch path


class Operands:
    """A case's operands on the device."""

    def __init__(self, case, refs, _hip, L, dev):
        from interactive_spectrogram_inpainting.vqvae import _ops
        self.case, self.refs, self.dev = case, refs, dev
        B, H, W = case.B, case.H, case.W
        p0, p1 = TS.VQ_FUSED_PARENTS if case.strided else (None, None)
        self.s0 = Source(_hip, L, refs.a0, B, H, W, dev, p0)
        self.s1 = Source(_hip, L, refs.a1, B, H, W, dev, p1) if refs.a1 is not None else None
        if case.strided:
            assert self.s0.strides != self.s1.strides and self.s0.offset != self.s1.offset and self.s1.offset > 0
        Cin = case.C0 + case.C1
        self.pw = _ops.pack_conv_weight(refs.W.reshape(D, Cin, 1, 1).to(dev), with_f16=True)
        self.n_packed = self.pw.numel() // 2
        self.Kpad = self.n_packed // D
        self.w16 = self.pw.data_ptr() + 4 * self.n_packed
        self.bias = refs.bias.to(dev)
        self.codes, self.e2 = _ops.pack_codebook(refs.embed.to(dev))
        self.ws_floats = L.isi_vq_conv1x1_workspace_floats(case.C0, case.C1, D)
        assert self.ws_floats == D * self.Kpad and self.Kpad == (Cin + 31) // 32 * 32
        torch.cuda.synchronize()
        self.inputs = [self.pw, self.bias, self.codes, self.e2]
        self.inputs_before = [t.clone() for t in self.inputs]

    def unchanged(self):
        srcs = [self.s0] + ([self.s1] if self.s1 is not None else [])
        return all(s.enc.untouched() for s in srcs) and all(_same(a, b) for a, b in zip(self.inputs, self.inputs_before))


class Outputs:
    def __init__(self, case, dev, K=None, garbage_counts=False):
        N, K = case.B * case.H * case.W, case.K if K is None else K
        self.N, self.K = N, K
        self.idx = Buf(N, dev, SENTINEL, torch.int64)
        self.q, self.q_pair, self.z = Buf(N * D, dev), Buf(N * D, dev), Buf(N * D, dev)
        g = torch.Generator().manual_seed(N + K)
        start = torch.randint(-1000, 1000, (K,), generator=g, dtype=torch.int32) if garbage_counts else torch.zeros(K, dtype=torch.int32)
        self.counts = Buf(K, dev, COUNT_GUARD, torch.int32, start)
        self.part = Buf(TS.vq_num_partials(N), dev)

    def all(self):
        return {"idx": self.idx, "q": self.q, "q_pair": self.q_pair, "z_out": self.z, "counts": self.counts, "sse_part": self.part}

    def assert_guards(self, what):
        for name, b in self.all().items():
            assert b.intact(), f"{what}: the kernel wrote outside {name}"

    def assert_untouched(self, what):
        for name, b in self.all().items():
            assert b.untouched(), f"{what}: a refused launch wrote to {name}"


def _launch(L, ops, out, ws, tape, q=True, q_pair=True, s0=None, s1=None, dims=None, D_=D, K=None):
    case = ops.case
    s0 = ops.s0.src if s0 is None else s0
    s1 = (ops.s1.src if ops.s1 is not None else None) if s1 is None else s1
    B, H, W = (case.B, case.H, case.W) if dims is None else dims
    head = (C.byref(s0), C.byref(s1) if s1 is not None else None, ops.w16, ops.bias.data_ptr(), ops.codes.data_ptr(),
            ops.e2.data_ptr(), out.idx.ptr, out.q.ptr if q else None, out.q_pair.ptr if q_pair else None)
    tail = (out.counts.ptr, out.part.ptr, ws, B, H, W, D_, out.K if K is None else K, None)
    if tape:
        rc = L.isi_vq_conv1x1_nearest_tape_f32(*head, out.z.ptr, *tail)
    else:
        rc = L.isi_vq_conv1x1_nearest_f32(*head, *tail)
    torch.cuda.synchronize()
    return rc


def _record(check):
    print(f"{check.what}: err {check.err:.3e} yardstick {check.yardstick:.3e} ratio {check.ratio:.3f}")
    RECORD.append(check)


def _check_row(what, got, ref, yard):
    err, y = TS.row_error(got, ref), max(TS.row_error(yard, ref), TS.ROW_OPS_FLOOR)
    RECORD.append(TS.RowCheck(what, err, y, err / y))                                   # (recorded whether it passes or not)
    print(f"{what}: err {err:.3e} yardstick {y:.3e} ratio {err / y:.3f}")
    TS.compare_rows(got, ref, yard, what)


def _hold_case(case, refs, name, two_launch=True):
    """The three launches of a case -- plain, tape, plain without q_out -- and every assertion on them."""
    _hip, L, dev = _lib()
    N, K, spec = case.B * case.H * case.W, case.K, refs.spec
    assert L.isi_vq_conv1x1_fusable(case.C0, case.C1, D, K) == 1
    n_part = L.isi_vq_num_partials(N)
    assert n_part == TS.vq_num_partials(N)
    ops = Operands(case, refs, _hip, L, dev)
    ws = Buf(ops.ws_floats, dev)

    plain, tape, noq = Outputs(case, dev), Outputs(case, dev, garbage_counts=True), Outputs(case, dev)
    assert _launch(L, ops, plain, ws.ptr, tape=False) == 0, L.isi_last_error()
    frag_plain = ws.view.clone()
    assert _launch(L, ops, tape, ws.ptr, tape=True) == 0, L.isi_last_error()
    assert _launch(L, ops, noq, ws.ptr, tape=False, q=False) == 0, L.isi_last_error()
    for o, which in ((plain, "plain"), (tape, "tape"), (noq, "no q_out")):
        o.assert_guards(f"{name} {which}")
    assert ws.intact(), f"{name}: the kernel wrote outside the workspace"
    assert ops.unchanged(), f"{name}: a launch changed one of its inputs"
    assert plain.z.untouched() and noq.z.untouched() and noq.q.untouched(), f"{name}: an output that was not asked for was written"

    # 1, 2: indices and histogram, all of them
    for o, which in ((plain, "plain"), (tape, "tape"), (noq, "no q_out")):
        TS.vq_fused_hold_idx(o.idx.cpu(), spec, f"{name} {which}")
        TS.vq_fused_hold_counts(o.counts.cpu(), spec, f"{name} {which}")
    # 3: z of the tape entry
    z = tape.z.cpu(N, D)
    live = spec.idx >= 0
    if bool(live.any()):
        _record(TS.vq_fused_hold_z(z, refs, name))
    # 4: q
    q = plain.q.cpu(N, D)
    TS.vq_fused_hold_q(q, refs, name)
    assert _same(plain.q.view, tape.q.view), f"{name}: q differs between the plain and the tape entry"
    TS.vq_fused_hold_q(tape.q.cpu(N, D), refs, f"{name} tape")
    # 5: the pair copy
    TS.vq_fused_hold_q_pair(plain.q_pair.cpu(N, D), q, refs, name)
    assert _same(plain.q_pair.view, noq.q_pair.view) and _same(plain.q_pair.view, tape.q_pair.view), \
        f"{name}: q_pair differs between the launches"
    # 6: the squared error and the scalars on top of it
    for o, which in ((plain, "plain"), (tape, "tape"), (noq, "no q_out")):
        TS.vq_fused_hold_sse(o.part.cpu(), spec, f"{name} {which}")
    if bool(live.all()):
        assert _same(plain.part.view, tape.part.view) and _same(plain.part.view, noq.part.view), f"{name}: sse_part differs between the launches"
        out2 = Buf(2, dev)
        assert L.isi_vq_finalize_f32(plain.part.ptr, n_part, plain.counts.ptr, K, N, D, out2.ptr, None) == 0, L.isi_last_error()
        torch.cuda.synchronize()
        assert out2.intact()
        part, counts = plain.part.cpu(), plain.counts.cpu()
        ref, yard = TS.vq_finalize_spec(part, counts, N, D), TS.vq_finalize_f32(part, counts, N, D)
        _check_row(f"{name} diff", out2.cpu()[0:1], ref[0], yard[0])
        _check_row(f"{name} perplexity", out2.cpu()[1:2], ref[1], yard[1])
        assert abs(float(out2.cpu()[0]) - float(spec.diff)) <= 2 * TS.VQ_FUSED_SSE_RTOL * float(spec.diff)
    # the workspace holds the fragment-major weight
    frag = Buf(ops.ws_floats, dev)
    assert L.isi_vq_pack_fragments_f32(ops.w16, frag.ptr, ops.Kpad, None) == 0, L.isi_last_error()
    torch.cuda.synchronize()
    assert frag.intact() and not bool(torch.isnan(frag.view).any())
    assert _same(frag.view, ws.view) and _same(frag.view, frag_plain), f"{name}: the workspace is not isi_vq_pack_fragments_f32's copy"
    # 7: the two-launch path on the same operands gives the same bits
    if two_launch and not case.strided:
        _hold_two_launches(_hip, L, dev, ops, tape, name)
    return plain, tape


def _hold_two_launches(_hip, L, dev, ops, tape, name):
    case = ops.case
    B, H, W, N, K = case.B, case.H, case.W, tape.N, tape.K

    def f32_src(s, Cc):
        return _hip.isi_src(s.dense_f32.ptr, Cc, H * W * Cc, 1, W * Cc, Cc)

    s0 = f32_src(ops.s0, case.C0)
    s1 = f32_src(ops.s1, case.C1) if ops.s1 is not None else None
    zc = Buf(N * D, dev)
    dst = _hip.isi_dst(zc.ptr, H * W * D, 1, W * D, D)
    rc = L.isi_conv2d_f32(C.byref(s0), C.byref(s1) if s1 is not None else None, ops.pw.data_ptr(), ops.bias.data_ptr(), None,
                          C.byref(dst), B, H, W, D, 1, 1, 1, 0, 8 | 16, None)
    assert rc == 0, L.isi_last_error()
    two = Outputs(case, dev)
    rc = L.isi_vq_nearest_flags_f32(zc.ptr, ops.codes.data_ptr(), ops.e2.data_ptr(), two.idx.ptr, two.q.ptr, two.counts.ptr,
                                    two.part.ptr, N, D, K, 8, None)
    assert rc == 0, L.isi_last_error()
    torch.cuda.synchronize()
    assert zc.intact()
    two.assert_guards(f"{name} two launches")
    assert _same(two.idx.view, tape.idx.view) and _same(two.counts.view, tape.counts.view), \
        f"{name}: the fused launch and convolution + search differ in idx or counts"
    if case.C0 + case.C1 >= 128:
        assert _same(zc.view, tape.z.view), f"{name}: z_out is not the stand-alone convolution's output bit for bit"
        assert _same(two.q.view, tape.q.view), f"{name}: the fused launch and convolution + search differ in q"
    else:
        # below 128 input channels the stand-alone convolution runs no split products at all (launch_conv of
        # csrc/conv_igemm_f32.hip keeps K < 128 on the exact-fp32 kernel, whatever the flags): its z is another rounding of
        # the same sum, held to the same spec, and q = z + (e - z) follows it
        _record(TS.vq_fused_hold_z(zc.cpu(N, D), ops.refs, f"{name} (exact-fp32 convolution)"))
        TS.vq_fused_hold_q(two.q.cpu(N, D), ops.refs, f"{name} (exact-fp32 convolution)")


# ----------------------------------------------------------------------------------------------------- channel routes
@pytest.mark.parametrize("case", TS.VQ_FUSED_ROUTE_CASES, ids=TS.vq_fused_case_id)
def test_channel_routes(case):
    chunks = (case.C0 + case.C1) // 32
    assert TS.VQ_FUSED_ROUTES[(case.C0, case.C1)] == 2 * ((chunks + 1) // 2), "the chunk-count template the case is named for"
    assert case.B * case.H * case.W == 257 and case.K == 512
    _hold_case(case, TS.vq_fused_case_refs(case), "routes " + TS.vq_fused_case_id(case))


# -------------------------------------------------------------------------------------------------------- pixel counts
@pytest.mark.parametrize("case", TS.VQ_FUSED_PIXEL_CASES, ids=TS.vq_fused_case_id)
def test_pixel_counts(case):
    _, L, _ = _lib()
    N = case.B * case.H * case.W
    if N > 65536:           # the second grid-stride pass: more tiles than workgroups
        assert L.isi_vq_num_partials(N) == TS.VQ_FUSED_GRID and -(-N // TS.VQ_FUSED_TILE) > TS.VQ_FUSED_GRID and N % TS.VQ_FUSED_TILE
    else:
        assert L.isi_vq_num_partials(N) == -(-N // TS.VQ_FUSED_TILE)
    _hold_case(case, TS.vq_fused_case_refs(case), "pixels " + TS.vq_fused_case_id(case))


# ------------------------------------------------------------------------------------------------------ codebook sizes
def _k_max(L):
    k_max = TS.vq_fused_k_max(L)
    assert L.isi_vq_conv1x1_fusable(64, 0, D, k_max) == 1 and L.isi_vq_conv1x1_fusable(64, 0, D, k_max + 1) == 0
    return k_max


@pytest.mark.parametrize("K", TS.VQ_FUSED_K_SIZES + ("K_max",))
def test_codebook_sizes(K):
    _, L, _ = _lib()
    k_max = _k_max(L)
    cases = TS.vq_fused_k_cases(k_max)
    case = cases[-1] if K == "K_max" else cases[TS.VQ_FUSED_K_SIZES.index(K)]
    assert case.K == (k_max if K == "K_max" else K) and k_max > 512 and k_max % 32 == 0
    _hold_case(case, TS.vq_fused_case_refs(case), "codebook " + TS.vq_fused_case_id(case))


def test_one_code_past_k_max_is_refused():
    _hip, L, dev = _lib()
    k_max = _k_max(L)
    case = TS.vq_fused_k_cases(k_max)[-1]
    refs = TS.vq_fused_case_refs(case)
    embed = torch.cat([refs.embed, refs.embed[:, :1] + 1.0], dim=1)
    ops = Operands(case, refs._replace(embed=embed), _hip, L, dev)
    assert ops.codes.shape == (k_max + 1, D)
    ws = Buf(ops.ws_floats, dev)
    for tape in (False, True):
        out = Outputs(case, dev, K=k_max + 1)
        assert _launch(L, ops, out, ws.ptr, tape=tape) == -4, "ISI_E_UNSUPPORTED"
        out.assert_untouched(f"K_max + 1, tape={tape}")
    assert ws.untouched() and ops.unchanged()


# ----------------------------------------------------------------------------------------------------- strided sources
@pytest.mark.parametrize("case", TS.VQ_FUSED_STRIDED_CASES, ids=TS.vq_fused_case_id)
def test_strided_sources(case):
    assert case.strided and (case.C0, case.C1) == (64, 128)
    _hold_case(case, TS.vq_fused_case_refs(case), "strided " + TS.vq_fused_case_id(case))


# ------------------------------------------------------------------------------------------------------ special values
def test_duplicate_codes_resolve_to_the_lowest_index():
    refs = TS.vq_fused_case_refs(ROUTE, dups=True)
    sources = torch.tensor(TS.VQ_FUSED_DUP_SOURCES)
    assert int(torch.isin(refs.spec.idx, sources).sum()) >= 3
    plain, tape = _hold_case(ROUTE, refs, "duplicates")
    for o in (plain, tape):
        idx = o.idx.cpu()
        for src, copies in zip(TS.VQ_FUSED_DUP_SOURCES, TS.VQ_FUSED_DUP_COPIES):
            assert int((idx == src).sum()) >= 1 and not bool(torch.isin(idx, torch.tensor(copies)).any())


def test_far_codes_inside_the_fused_kernel():
    refs = TS.vq_fused_refs(*TS.vq_fused_far_case_data(ROUTE))
    for pixel, code in TS.VQ_FUSED_FAR_PIXELS.items():
        assert int(refs.spec.idx[pixel]) == code
    plain, tape = _hold_case(ROUTE, refs, "far codes")
    for pixel, code in TS.VQ_FUSED_FAR_PIXELS.items():
        assert int(plain.idx.cpu()[pixel]) == code and int(tape.idx.cpu()[pixel]) == code


def test_non_finite_code_is_loud():
    r = TS.vq_fused_case_refs(ROUTE)
    embed = r.embed.clone()
    embed[3, 100] = float("inf")
    refs = TS.vq_fused_refs(r.a0, r.a1, r.W, r.bias, embed)
    assert bool((refs.spec.idx == -1).all())
    plain, tape = _hold_case(ROUTE, refs, "non-finite code", two_launch=False)
    for o in (plain, tape):
        assert bool((o.idx.cpu() == -1).all()) and int(o.counts.cpu().abs().sum()) == 0
        assert bool(torch.isnan(o.part.cpu().double().sum())) and bool(torch.isnan(o.q.cpu()).all())


def _lost_pixels_case(value, name):
    r = TS.vq_fused_case_refs(ROUTE)
    a0, a1 = r.a0.clone(), r.a1.clone()
    a0[70, 37], a1[256, 101] = value, value               # one in each source; pixel 256 is the ragged tile's only one
    refs = TS.vq_fused_refs(a0, a1, r.W, r.bias, r.embed)
    lost = torch.zeros(257, dtype=torch.bool)
    lost[[70, 256]] = True
    assert torch.equal(refs.spec.idx < 0, lost) and torch.equal(refs.spec.idx[~lost], r.spec.idx[~lost])
    plain, tape = _hold_case(ROUTE, refs, name, two_launch=False)
    for o in (plain, tape):
        idx, q = o.idx.cpu(), o.q.cpu(257, D)
        assert torch.equal(idx < 0, lost) and torch.equal(idx[~lost], r.spec.idx[~lost])
        assert bool(torch.isnan(q[lost]).all()) and bool(torch.isfinite(q[~lost]).all())
        assert int(o.counts.cpu().sum()) == 255 and bool(torch.isnan(o.part.cpu().double().sum()))


def test_nan_activation_is_loud():
    _lost_pixels_case(float("nan"), "NaN activation")


def test_activation_beyond_the_pair_range_is_loud():
    _lost_pixels_case(3.0e4, "activation beyond 16384")


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    _hip, L, dev = _lib()
    case, refs = ROUTE, TS.vq_fused_case_refs(ROUTE)
    ops = Operands(case, refs, _hip, L, dev)
    ws = Buf(ops.ws_floats + 4, dev)
    out = Outputs(case, dev)

    def src(s, **over):
        f = {"ptr": s.src.ptr, "C": s.src.C, "sn": s.src.sn, "sc": s.src.sc, "sh": s.src.sh, "sw": s.src.sw}
        f.update(over)
        return _hip.isi_src(f["ptr"], f["C"], f["sn"], f["sc"], f["sh"], f["sw"])

    refused = {
        "sc != 1 (first source)": dict(s0=src(ops.s0, sc=2)),
        "sc != 1 (second source)": dict(s1=src(ops.s1, sc=192)),
        "C0 = 48": dict(s0=src(ops.s0, C=48)),
        "C0 + C1 = 288": dict(s0=src(ops.s0, C=160)),
        "D = 32": dict(D_=32),
        "misaligned workspace": dict(ws=ws.ptr + 4),
        "q_out and q_pair_out both NULL": dict(q=False, q_pair=False),
        "no pixels": dict(dims=(1, 0, 257)),
    }
    for tape in (False, True):
        for what, kw in refused.items():
            kw = dict(kw)
            rc = _launch(L, ops, out, kw.pop("ws", ws.ptr), tape=tape, **kw)
            assert rc in (-1, -4), f"{what}: returned {rc}"
            out.assert_untouched(f"{what}, tape={tape}")
            assert ws.untouched() and ops.unchanged(), what
    # the same operands are accepted as they stand
    assert _launch(L, ops, out, ws.ptr, tape=False) == 0, L.isi_last_error()
    TS.vq_fused_hold_idx(out.idx.cpu(), refs.spec, "refusals: the accepted launch")
