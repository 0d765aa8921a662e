"""The relative-attention forward (isi_rel_attention_f32 through ctypes) against its float64 specification on every
route: the exact-fp32 kernel, the 64-key-tile 16-bit kernels, the plane-staged 16-bit kernel and, behind the two, the
one-row tail kernel (tests/tests_support.py: attention_fwd_spec, the float32 yardstick, the 16-bit operand models, the
case table and its requirements; tests/test_attention_fwd_host.py shows what the hold rejects).

Held with compare_rows, ROW_OPS_MARGIN and ROW_OPS_FLOOR: out, the log-sum-exp and the kept base-2 logits; empty rows are
out = 0 and lse = 1e30 exactly, -inf logits -inf exactly.

Every device buffer sits between NaN pads, outputs and the workspace start as NaN, the gaps of the strided layouts and the
foreign thirds of a fused [S,B,3d] buffer hold NaN: a finite, correct result proves that the right elements were read,
untouched pads and gaps that nothing else was written.  Plane-staged and persistent cases run twice and must repeat bit
for bit (profiles/r06_attention_skew_race.txt); where a knob switches the kernel the two results must differ.

With ISI_ATTENTION_FWD_RECORD=<file> the worst ratio per family and output is also written there
(profiles/attention_fwd_checks.txt)."""
import collections
import contextlib
import ctypes as C
import os
import time

import pytest
import torch

import tests_support as T

pytestmark = pytest.mark.gpu

PAD = 64
RECORD = collections.defaultdict(list)      # (family, output) -> [RowCheck]
CASES = T.ATTENTION_FWD_CASES
IDS = [T.attention_fwd_case_id(c) for c in CASES]
NAN = float("nan")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def _record():
    t0 = time.time()
    yield
    lines = []
    for (family, output), checks in sorted(RECORD.items()):
        w = max(checks, key=lambda r: r.ratio)
        lines.append(f"RECORD attention_fwd {family} {output}: worst error / yardstick {w.ratio:.3f} over {len(checks)} comparisons "
                     f"(err {w.err:.3e}, yardstick {w.yardstick:.3e}, {w.what})")
    lines.append(f"RECORD attention_fwd wall time: {time.time() - t0:.1f} s, the float64 references included")
    print("\n" + "\n".join(lines))
    path = os.environ.get("ISI_ATTENTION_FWD_RECORD")
    if path and RECORD:
        head = ("# tests/test_attention_fwd_gpu.py on an MI355X (ISI_ATTENTION_FWD_RECORD): per kernel family (tail: the one-row kernel behind a\n"
                "# 16-bit kernel) and output the worst ratio of the kernel's error to the yardstick's, both against the float64 spec.  Yardstick:\n"
                "# the float32 evaluation; on the tile rows of the 16-bit modes per element the worse of it and the mode's operand model\n"
                "# (tests_support.attention_fwd_refs).  Metric and bound: tests_support.compare_rows (ratio <= 8); no term was added to a yardstick.\n")
        with open(path, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


def _settle(rc, what):
    """Wait for the launch.  A launch failure or a device error is no comparison that failed: the session ends there, so that
    nothing more is started on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: the device reported {e}", returncode=3)
    if rc == -2:                 # ISI_E_LAUNCH
        from interactive_spectrogram_inpainting import _hip
        pytest.exit(f"{what}: launch failure: {_hip.lib().isi_last_error()}", returncode=3)


class Region:
    """n floats of NaN on the device between NaN pads of PAD floats; strided views into it; what is still NaN afterwards."""

    def __init__(self, n, dev):
        self.n = n
        self.full = torch.full((n + 2 * PAD,), NAN, dtype=torch.float32, device=dev)
        self.t = self.full[PAD:PAD + n]
        self.ptr = self.t.data_ptr()
        assert self.ptr % 256 == 0

    def view(self, sizes, strides, off=0):
        assert off + sum((n - 1) * s for n, s in zip(sizes, strides)) < self.n
        return torch.as_strided(self.t, sizes, strides, self.t.storage_offset() + off)

    def pads_intact(self):
        return bool(torch.isnan(self.full[:PAD]).all()) and bool(torch.isnan(self.full[-PAD:]).all())

    def untouched_outside(self, *views):
        """every element outside the given views (made by self.view) is still NaN"""
        inside = torch.zeros(self.n, dtype=torch.bool, device=self.t.device)
        for sizes, strides, off in views:
            torch.as_strided(inside, sizes, strides, off).fill_(True)
        return bool(torch.isnan(self.t[~inside]).all())


def _strides(layout, S, B, H, hd, third=0):
    """(ss, sb, sh), offset and floats of a [S,B,H,hd] tensor in a buffer layout"""
    d = H * hd
    if layout == "contig":
        return (B * d, d, hd), 0, S * B * d
    if layout == "fused":                       # a third of a [S,B,3d] buffer
        return (B * 3 * d, 3 * d, hd), third * d, S * B * 3 * d
    if layout == "batch_first":
        return (d, S * d, hd), 0, B * S * d
    if layout == "head2":                       # a gap of hd floats behind every head
        return (B * H * 2 * hd, H * 2 * hd, 2 * hd), 0, S * B * H * 2 * hd
    assert layout == "wide", layout             # rows of d + 8 floats
    return (B * (d + 8), d + 8, hd), 0, S * B * (d + 8)


class Inputs:
    """The device buffers a case reads, built once per case: q, k, v in the case's layout (one shared [S,B,3d] buffer for
    "fused" when Sq = Sk, else one buffer each with the foreign thirds left NaN), the table and the dense mask."""

    def __init__(self, c, d, dev):
        self.c, self.d, self.dev = c, d, dev
        self.regions, self.views, self.at = [], {}, {}
        shared = None
        for third, (name, data, S) in enumerate((("q", d.q, c.Sq), ("k", d.k, c.Sk), ("v", d.v, c.Sk))):
            st, off, n = _strides(c.layout, S, c.B, c.H, c.hd, third)
            if c.layout == "fused" and c.Sq == c.Sk:
                shared = shared or self._region(n)
                reg = shared
            else:
                reg = self._region(n)
            view = reg.view((S, c.B, c.H, c.hd), st + (1,), off)
            view.copy_(data)
            self.views[name], self.at[name] = view, (reg.ptr + 4 * off, st)
        self.rel = self._filled(d.rel)
        self.dense = self._filled(d.dense)

    def _region(self, n):
        self.regions.append(Region(n, self.dev))
        return self.regions[-1]

    def _filled(self, data):
        if data is None:
            return None
        reg = self._region(data.numel())
        reg.t.copy_(data.reshape(-1))
        return reg

    def intact(self):
        return all(r.pads_intact() for r in self.regions)


Result = collections.namedtuple("Result", "fwd workspace_written")


def _knobs(bits):
    from interactive_spectrogram_inpainting import _hip
    stack = contextlib.ExitStack()
    for bit, name in T.ATTN_KNOB_NAMES.items():
        if bits & bit:
            stack.enter_context(_hip.knob(name, 1))
    return stack


def _workspace(c, a, dev, family):
    """The workspace the case hands over, as the code offers it: "query" asks the size query under the case's knobs (it must
    answer exactly when the plane-staged kernel takes the call); "given" brings the plane-staged kernel's size -- asked under
    ISI_ATTN_FWD3_ALL, without which the query declines the single-term modes -- or 4 KiB where that kernel never takes the
    call."""
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    if c.ws == "none":
        return None
    if c.ws == "query":
        with _knobs(c.knobs):
            need = L.isi_rel_attention_workspace_bytes(C.byref(a))
        assert (need > 0) == (family == "planes"), f"size query {need} on a {family} route"
        return Region(need // 4, dev) if need else None
    with _knobs(T.ATTN_KNOB_FWD3_ALL):
        need = L.isi_rel_attention_workspace_bytes(C.byref(a))
    assert (need > 0) == (family == "planes")
    return Region((need or 4096) // 4, dev)


def _launch(c, inp, family, extra_knobs=0, contiguous_out=False):
    """One call of isi_rel_attention_f32 on fresh NaN outputs; the results on the CPU as the spec lays them out, after the
    integrity checks of every buffer."""
    from interactive_spectrogram_inpainting import _hip
    d, dev = inp.d, inp.dev
    what = T.attention_fwd_case_id(c)
    a = _hip.isi_attn_args()
    a.q, (a.q_ss, a.q_sb, a.q_sh) = inp.at["q"]
    a.k, (a.k_ss, a.k_sb, a.k_sh) = inp.at["k"]
    a.v, (a.v_ss, a.v_sb, a.v_sh) = inp.at["v"]
    a.rel_embeddings = inp.rel.ptr if inp.rel else None
    a.dense_mask = inp.dense.ptr if inp.dense else None
    a.Sq, a.Sk, a.B, a.H, a.head_dim = c.Sq, c.Sk, c.B, c.H, c.hd
    a.Cq, a.Ck, a.Ek, a.rel_rows = c.Cq, c.Ck, d.Ek, d.rel_rows if d.rel is not None else 0
    a.mask_mode, a.scale, a.precision = c.mask, d.scale, c.prec
    ost, ooff, on = _strides("wide" if c.wide and not contiguous_out else "contig", c.Sq, c.B, c.H, c.hd)
    out = Region(on, dev)
    a.out, (a.o_ss, a.o_sb, a.o_sh) = out.ptr, ost
    lse = logits = None
    if c.outputs != "none":
        lse = Region(c.B * c.H * c.Sq, dev)
        a.lse = lse.ptr
    ld = (c.Sk + 31) // 32 * 32 + c.ld_extra
    if c.outputs == "lse+logits":
        logits = Region(c.B * c.H * c.Sq * ld, dev)
        a.logits, a.logits_ld = logits.ptr, ld
    ws = _workspace(c, a, dev, family if not extra_knobs & T.ATTN_KNOB_NO_FWD3 else "planes")
    if ws is not None:
        a.workspace, a.workspace_bytes = ws.ptr, ws.n * 4
    with _knobs(c.knobs | extra_knobs):
        rc = _hip.lib().isi_rel_attention_f32(C.byref(a), _hip.stream_ptr(dev))
    _settle(rc, what)
    assert rc == 0, f"{what}: refused with {rc}: {_hip.lib().isi_last_error()}"
    oview = (c.Sq, c.B, c.H, c.hd), ost + (1,), ooff
    assert inp.intact(), f"{what}: a pad of an input was written"
    assert out.pads_intact() and out.untouched_outside(oview), f"{what}: out was written outside its elements"
    assert lse is None or lse.pads_intact(), f"{what}: the pads of lse were written"
    assert logits is None or logits.pads_intact(), f"{what}: the pads of the kept logits were written"
    assert ws is None or ws.pads_intact(), f"{what}: the pads of the workspace were written"
    fwd = T.AttnFwd(out.view(*oview).permute(1, 2, 0, 3).cpu(), None if lse is None else lse.t.view(c.B, c.H, c.Sq).cpu(),
                    None if logits is None else logits.t.view(c.B, c.H, c.Sq, ld).cpu(), None)
    return Result(fwd, None if ws is None else not bool(torch.isnan(ws.t).all()))


def _same_bits(x, y, allowed):
    if not T.same_bits(x.out, y.out) or (x.lse is not None and not T.same_bits(x.lse, y.lse)):
        return False
    if x.logits2 is None:
        return True
    Sk = allowed.shape[1]
    keep = allowed.expand_as(x.logits2[..., :Sk])
    return T.same_bits(x.logits2[..., :Sk][keep], y.logits2[..., :Sk][keep])


def _hold(family, got, refs, what):
    checks = T.attention_fwd_hold(got, refs, what)
    for output, r in checks.items():
        RECORD[("tail", output[5:]) if output.startswith("tail ") else (family, output)].append(r)
    return checks


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_attention_forward_against_spec(c):
    cus = _cus()
    family, tail, nW = T.attention_fwd_case_route(c, cus)
    r, d, refs = T.attention_fwd_case_refs(c, cus)
    assert refs.tail == tail
    what = T.attention_fwd_case_id(r)
    inp = Inputs(r, d, _dev())
    got = _launch(r, inp, family)
    # the route, as far as a call shows it: the plane-staged kernel's pack launch writes the workspace, nothing else does
    assert got.workspace_written in (None, family == "planes"), f"{what}: predicted {family}, workspace written: {got.workspace_written}"
    _hold(family, got.fwd, refs, what)
    if family == "planes" or c.persistent:
        again = _launch(r, inp, family)
        assert _same_bits(got.fwd, again.fwd, refs.spec.allowed), f"{what}: two launches differ"
    if family == "planes" and not c.persistent:
        # ISI_ATTN_NO_FWD3 on the same call: the 64-key tiles, which leave the workspace alone.  The two kernels multiply the
        # same operands; they deal a block's keys to their two wave groups differently -- the tiles in alternating runs of KT
        # keys (rel_attention_fwd2.hip: Tile::KT), the planes in two contiguous halves -- so with more than two runs
        # of keys in some block the sums are formed in another order and the outputs must differ in some bit
        other = _launch(r, inp, "tiles64", extra_knobs=T.ATTN_KNOB_NO_FWD3)
        assert other.workspace_written is False, f"{what}: ISI_ATTN_NO_FWD3 still wrote the workspace"
        KT = 32 if (c.prec == 1 and c.hd == 64) else 64
        if (min(c.Sk, c.Sq) if c.mask == 1 else c.Sk) > 2 * KT and c.Sq >= 127 and c.kind != "flat":
            assert not T.same_bits(other.fwd.out, got.fwd.out), f"{what}: ISI_ATTN_NO_FWD3 changed no bit of the output"
        _hold("tiles64", other.fwd, refs, what + " under ISI_ATTN_NO_FWD3")


@pytest.mark.parametrize("c", T.ATTENTION_FWD_ENTRY_CASES, ids=[T.attention_fwd_case_id(c) for c in T.ATTENTION_FWD_ENTRY_CASES])
def test_python_entry_equals_the_direct_call(c, monkeypatch):
    """_ops.rel_attention on the same views (strides, the size query, the workspace) bit for bit."""
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    family, _, _ = T.attention_fwd_case_route(c, _cus())
    r, d, refs = T.attention_fwd_case_refs(c, _cus())
    inp = Inputs(r, d, dev)
    direct = _launch(r, inp, family, contiguous_out=True).fwd
    monkeypatch.setattr(_ops, "ATTENTION_PRECISION", {v: k for k, v in _ops._ATTN_PREC.items()}[c.prec])
    dm = c.H * c.hd
    q, k, v = (inp.views[n].flatten(2) if inp.views[n].stride(2) == c.hd else None for n in "qkv")
    assert q is not None and q.shape == (c.Sq, c.B, dm) and q.data_ptr() == inp.at["q"][0]
    ld = (c.Sk + 31) // 32 * 32
    lse = torch.full((c.B, c.H, c.Sq), NAN, device=dev)
    logits = torch.full((c.B, c.H, c.Sq, ld), NAN, device=dev)
    with _knobs(c.knobs):
        out = _ops.rel_attention(q, k, v, None if inp.rel is None else inp.rel.t.view(c.H, d.rel_rows, c.hd), c.H, c.Cq, c.Ck, d.Ek,
                                 mask_mode=c.mask, dense_mask=None if inp.dense is None else inp.dense.t.view(c.Sq, c.Sk), lse=lse,
                                 logits=logits)
    _settle(0, T.attention_fwd_case_id(c))
    got = T.AttnFwd(out.view(c.Sq, c.B, c.H, c.hd).permute(1, 2, 0, 3).cpu(), lse.cpu(), logits.cpu(), None)
    assert _same_bits(got, direct, refs.spec.allowed)
