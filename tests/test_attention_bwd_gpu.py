"""The relative-attention backward (isi_rel_attention_bwd_f32 through ctypes) against its float64 specification on every
route of csrc/rel_attention_run.cpp's BwdRoute: the exact-fp32 pair and the split pair, three-term and single-term
products, recomputed and kept logits, dQ += G E on the banded GEMM and on the batched 1x1 convolution, G zeroed in full
and in the margins of its band, g_from_kv with its two launches, the one-row and one-key tails, the halved table rows of
the causal masks (tests/tests_support.py: attention_bwd_spec, the float32 yardstick, the split pair's operand model, the
route mirror, the case table and its requirements; tests/test_attention_bwd_host.py shows what the hold rejects).

The backward is handed out, lse and kept logits that come from the float64 forward specification, not from a kernel: an
error of the project's forward cannot absorb one of the backward.  Held with compare_rows, ROW_OPS_MARGIN and
ROW_OPS_FLOOR per output (dq, dk, dv, d_rel); rows the spec finds exactly 0 are 0.

Every device buffer sits between NaN pads; dq, dk, dv, d_rel and the WHOLE workspace start as NaN, the gaps of the strided
layouts and the foreign thirds of a fused [S,B,3d] buffer hold NaN, as do the kept logits of every pair the mask leaves out:
a finite, correct result proves that the right elements were read, untouched pads and gaps that nothing else was written.
What is still NaN in G afterwards shows which zeroing the library really ran.  Every case runs twice on fresh buffers.

With ISI_ATTENTION_BWD_RECORD=<file> the worst ratio per route family and output is also written there
(profiles/attention_bwd_checks.txt)."""
import collections
import contextlib
import ctypes as C
import os
import time
import types

import pytest
import torch

import tests_support as T
from test_attention_fwd_gpu import NAN, Inputs, Region, _cus, _dev, _settle, _strides

pytestmark = pytest.mark.gpu

RECORD = collections.defaultdict(list)      # (route family, output) -> [RowCheck]
CASES = T.ATTENTION_BWD_CASES
IDS = [T.attention_bwd_case_id(c) for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _record():
    t0 = time.time()
    yield
    lines = []
    for (family, output), checks in sorted(RECORD.items()):
        w = max(checks, key=lambda r: r.ratio)
        lines.append(f"RECORD attention_bwd {family} {output}: worst error / yardstick {w.ratio:.3f} over {len(checks)} comparisons "
                     f"(err {w.err:.3e}, yardstick {w.yardstick:.3e}, {w.what})")
    lines.append(f"RECORD attention_bwd wall time: {time.time() - t0:.1f} s, the float64 references included")
    print("\n" + "\n".join(lines))
    path = os.environ.get("ISI_ATTENTION_BWD_RECORD")
    if path and RECORD:
        head = ("# tests/test_attention_bwd_gpu.py on an MI355X (ISI_ATTENTION_BWD_RECORD): per route family -- kernel pair (exact | split: logits\n"
                "# recomputed | saved: kept logits), the products over G (no table | conv: 1x1 convolution | gemm: banded GEMM; G zeroed in full |\n"
                "# in its margins | margins + g_from_kv), `tail`: the rows of the one-row / one-key kernels -- and output the worst ratio of the\n"
                "# kernel's error to the yardstick's, both against the float64 spec.  Yardstick: the float32 evaluation; on the split routes per\n"
                "# element the worse of it and the operand model (tests_support.attention_bwd_refs).  Metric and bound: tests_support.compare_rows\n"
                "# (ratio <= 8); no term was added to a yardstick.\n")
        with open(path, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


def _family(c, route):
    g = ("no table" if not route.has_e else
         ("gemm" if route.gemm_path else "conv") + (" g_from_kv" if route.g_from_kv else " margins" if route.band_only else " full zero"))
    return f"{T.attention_bwd_family(c)}, {g}"


def _knobs(bits):
    from interactive_spectrogram_inpainting import _hip
    stack = contextlib.ExitStack()
    for bit, (name, value) in T.ATTN_BWD_KNOBS.items():
        if bits & bit:
            stack.enter_context(_hip.knob(name, value))
    return stack


class Given:
    """The device buffers a case reads besides q, k, v, the table and the mask (Inputs): out and dO in one layout (rows of
    d + 8 floats for a `wide` case), lse, and the kept logits with their NaN entries."""

    def __init__(self, c, d, route, dev):
        self.ost, self.ooff, on = _strides("wide" if c.wide else "contig", c.Sq, c.B, c.H, c.hd)
        self.out, self.dout = Region(on, dev), Region(on, dev)
        for reg, data in ((self.out, d.out), (self.dout, d.dout)):
            reg.view((c.Sq, c.B, c.H, c.hd), self.ost + (1,), self.ooff).copy_(data)
        self.lse = Region(c.B * c.H * c.Sq, dev)
        self.lse.t.copy_(d.lse.reshape(-1))
        self.logits = None
        if route.saved:
            self.logits = Region(d.logits.numel(), dev)
            self.logits.t.copy_(d.logits.reshape(-1))
        self.regions = [r for r in (self.out, self.dout, self.lse, self.logits) if r is not None]

    def intact(self):
        return all(r.pads_intact() for r in self.regions)


Result = collections.namedtuple("Result", "bwd g_nan")


def _call(c, d, route, at, given_ptrs, out_at, drel_ptr, ws, what):
    """isi_rel_attention_bwd_f32 on explicit pointers: at / out_at = {"q" | "k" | "v": (pointer, (ss, sb, sh))} of the inputs and
    of dq | dk | dv (same strides), given_ptrs = (out, dO, their strides, lse, logits or None, ld)."""
    from interactive_spectrogram_inpainting import _hip
    a = _hip.isi_attn_bwd_args()
    f = a.fwd
    f.q, (f.q_ss, f.q_sb, f.q_sh) = at["q"]
    f.k, (f.k_ss, f.k_sb, f.k_sh) = at["k"]
    f.v, (f.v_ss, f.v_sb, f.v_sh) = at["v"]
    assert all(out_at[n][1] == at[n][1] for n in "qkv")
    f.rel_embeddings, f.dense_mask = at.get("rel"), at.get("dense")
    f.Sq, f.Sk, f.B, f.H, f.head_dim = c.Sq, c.Sk, c.B, c.H, c.hd
    f.Cq, f.Ck, f.Ek, f.rel_rows = c.Cq, c.Ck, d.Ek, d.rel_rows if d.rel is not None else 0
    f.mask_mode, f.scale, f.precision = c.mask, d.scale, c.prec
    f.out, a.d_out, (f.o_ss, f.o_sb, f.o_sh), f.lse, logits, ld = given_ptrs
    if logits is not None:
        f.logits, f.logits_ld = logits, ld
    a.dq, a.dk, a.dv, a.d_rel = out_at["q"][0], out_at["k"][0], out_at["v"][0], drel_ptr
    # the mirror's premises, from what is really handed over
    assert (f.q_ss == c.B * f.q_sb) == (c.layout != "batch_first"), what
    need = _hip.lib().isi_rel_attention_bwd_workspace_floats(C.byref(f))
    assert need >= route.g_off + route.g_len, f"{what}: the size query answers {need}, G alone ends at {route.g_off + route.g_len}"
    if ws is None:
        return need
    assert ws.n == need                     # exactly the queried size
    a.workspace, a.workspace_floats = ws.ptr, need
    with _knobs(c.knobs):
        rc = _hip.lib().isi_rel_attention_bwd_f32(C.byref(a), _hip.stream_ptr(_dev()))
    _settle(rc, what)
    assert rc == 0, f"{what}: refused with {rc}: {_hip.lib().isi_last_error()}"
    return need


def _launch(c, d, route, inp, given):
    """One call on fresh NaN outputs and a fresh NaN workspace; the results on the CPU as the spec lays them out, after the
    integrity checks of every buffer, and where G is NaN afterwards ([H,Sq,B,Rp], None without a table)."""
    dev = inp.dev
    what = T.attention_bwd_case_id(c)
    regions, out_at, views, own, shared = [], {}, collections.defaultdict(list), {}, None
    for third, (name, S) in enumerate((("q", c.Sq), ("k", c.Sk), ("v", c.Sk))):
        st, off, n = _strides(c.layout, S, c.B, c.H, c.hd, third)
        if c.layout == "fused" and c.Sq == c.Sk:
            shared = shared or Region(n, dev)
            reg = shared
        else:
            reg = Region(n, dev)
        if not any(reg is r for r in regions):
            regions.append(reg)
        out_at[name] = (reg.ptr + 4 * off, st)
        own[name] = (reg, ((S, c.B, c.H, c.hd), st + (1,), off))
        views[id(reg)].append(own[name][1])
    drel = Region(c.H * d.rel_rows * c.hd, dev) if d.rel is not None else None
    at = dict(inp.at, rel=inp.rel.ptr if inp.rel else None, dense=inp.dense.ptr if inp.dense else None)
    ptrs = (given.out.ptr, given.dout.ptr, given.ost, given.lse.ptr, given.logits.ptr if given.logits else None, d.ld)
    need = _call(c, d, route, at, ptrs, out_at, drel.ptr if drel else None, None, what)
    ws = Region(need, dev)
    _call(c, d, route, at, ptrs, out_at, drel.ptr if drel else None, ws, what)
    assert inp.intact() and given.intact(), f"{what}: a pad of an input was written"
    for reg in regions:
        assert reg.pads_intact() and reg.untouched_outside(*views[id(reg)]), f"{what}: dq | dk | dv was written outside its elements"
    assert drel is None or drel.pads_intact(), f"{what}: the pads of d_rel were written"
    assert ws.pads_intact(), f"{what}: the pads of the workspace were written"
    get = lambda name: own[name][0].view(*own[name][1]).permute(1, 2, 0, 3).cpu()
    bwd = T.AttnBwd(get("q"), get("k"), get("v"), None if drel is None else drel.t.view(c.H, d.rel_rows, c.hd).cpu())
    g_nan = None
    if route.has_e:
        g_nan = torch.isnan(ws.t[route.g_off:route.g_off + route.g_len]).view(c.H, c.Sq, c.B, route.Rp).cpu()
    return Result(bwd, g_nan)


def _far_from_band(route, Sq):
    """[Sq,Rp]: the elements of G the margins kernel leaves alone: further than kMargin from the row's band, the margins
    rounded outwards to whole quads as attn_zero_margins_kernel stores them (`a0`, `b1`)."""
    ls, lb, hs, hb = route.band
    i, col = torch.arange(Sq)[:, None], torch.arange(route.Rp)[None, :]
    lo, hi = ls * i + lb, hs * i + hb
    a0 = (lo - T.ATTN_G_MARGIN).clamp(min=0) // 4 * 4
    b1 = ((hi + 1 + T.ATTN_G_MARGIN).clamp(max=route.Rp).clamp(min=0) + 3) // 4 * 4
    return (col < a0) | (col >= b1)


def _check_zeroing(c, route, g_nan, what):
    """Route evidence: which zeroing ran, from a workspace that started as NaN.  Margins only: what lies further than kMargin
    from a row's band is still NaN (and everything nearer was zeroed or stored); in full: nothing is."""
    if g_nan is None:
        return
    if not route.band_only:
        assert not bool(g_nan.any()), f"{what}: the mirror predicts G zeroed in full, {int(g_nan.sum())} elements are still NaN"
        return
    far = _far_from_band(route, c.Sq)
    per_row = g_nan.permute(0, 2, 1, 3)                      # [H,B,Sq,Rp]
    assert bool(per_row[:, :, far].all()), f"{what}: the mirror predicts margins-only zeroing, G was written far from its band"
    assert not bool(per_row[:, :, ~far].any()), f"{what}: an element of G's band or margins is still NaN"
    if c.Sq > 2 * T.ATTN_G_MARGIN + 1:
        assert bool(far.any()), f"{what}: no element of G lies beyond the margins"


def _same_bits(x, y, c):
    """dK and dV on every route; dQ and dE where every element of G receives at most one term (include/isi_hip.h)"""
    names = ["dk", "dv"] + (["dq", "d_rel"] if c.Ck == 1 or not c.table else [])
    return [n for n in names if getattr(x, n) is not None and not T.same_bits(getattr(x, n), getattr(y, n))]


def _hold(c, route, got, refs, what):
    checks = T.attention_bwd_hold(got, refs, what)
    for output, r in checks.items():
        RECORD[("tail", output[5:]) if output.startswith("tail ") else (_family(c, route), output)].append(r)
    return checks


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_attention_backward_against_spec(c):
    cus = _cus()
    route = T.attention_bwd_case_route(c, cus)
    r, d, refs = T.attention_bwd_case_refs(c, cus)
    assert refs.route == route
    what = T.attention_bwd_case_id(r)
    inp, given = Inputs(r, d, _dev()), Given(r, d, route, _dev())
    got = _launch(r, d, route, inp, given)
    _check_zeroing(r, route, got.g_nan, what)
    _hold(r, route, got.bwd, refs, what)
    again = _launch(r, d, route, inp, given)
    assert _same_bits(got.bwd, again.bwd, r) == [], f"{what}: two launches differ"
    _check_zeroing(r, route, again.g_nan, what)


@pytest.mark.parametrize("c", T.ATTENTION_BWD_ENTRY_CASES, ids=[T.attention_bwd_case_id(c) for c in T.ATTENTION_BWD_ENTRY_CASES])
def test_python_entry_equals_the_direct_call(c, monkeypatch):
    """RelAttentionFn.backward with its forward's saved tensors replaced by the case's spec-derived out, lse and kept logits:
    the strides of the q | k | v slices, the workspace query and the logits plumbing of priors/_train.py, bit for bit the
    direct call on the same buffers (fused: a = qkv [S,B,3d]; contiguous: a = q [Sq,B,d], b = k|v [Sk,B,2d])."""
    from interactive_spectrogram_inpainting.priors import _ops, _train
    dev = _dev()
    route = T.attention_bwd_case_route(c, _cus())
    r, d, refs = T.attention_bwd_case_refs(c, _cus())
    what = T.attention_bwd_case_id(r)
    dm = c.H * c.hd
    flat = lambda t: t.reshape(t.shape[0], c.B, dm)
    if c.layout == "fused":
        a_in, b_in = torch.cat([flat(d.q), flat(d.k), flat(d.v)], dim=-1).to(dev), None
    else:
        a_in, b_in = flat(d.q).to(dev), torch.cat([flat(d.k), flat(d.v)], dim=-1).to(dev)
    rel = None if d.rel is None else d.rel.to(dev)
    dense = None if d.dense is None else d.dense.to(dev)
    out, dout, lse, logits = flat(d.out).to(dev), flat(d.dout).to(dev), d.lse.to(dev), d.logits.to(dev)
    name = {v: k for k, v in _ops._ATTN_PREC.items()}[c.prec]
    ctx = types.SimpleNamespace(saved_tensors=(a_in, b_in, rel, out, lse, dense, logits), cfg=(c.H, c.Cq, c.Ck, d.Ek, c.mask, name))
    monkeypatch.setattr(_train.RelAttentionFn, "workspace_fill", NAN)
    da, db, drel = _train.RelAttentionFn.backward(ctx, dout)[:3]
    _settle(0, what)
    # the direct call on the same input buffers, outputs of the same shapes
    q, k, v = _train.RelAttentionFn._split(a_in, b_in)
    da2 = torch.full_like(a_in, NAN)
    db2 = None if b_in is None else torch.full_like(b_in, NAN)
    dq, dk, dv = _train.RelAttentionFn._split(da2, db2)
    drel2 = None if rel is None else torch.full_like(rel, NAN)
    at = {n: (t.data_ptr(), (t.stride(0), t.stride(1), c.hd)) for n, t in (("q", q), ("k", k), ("v", v))}
    at.update(rel=None if rel is None else rel.data_ptr(), dense=None if dense is None else dense.data_ptr())
    out_at = {n: (t.data_ptr(), (t.stride(0), t.stride(1), c.hd)) for n, t in (("q", dq), ("k", dk), ("v", dv))}
    ptrs = (out.data_ptr(), dout.data_ptr(), (out.stride(0), out.stride(1), c.hd), lse.data_ptr(), logits.data_ptr(), logits.stride(2))
    args = (r, d, route, at, ptrs, out_at, None if drel2 is None else drel2.data_ptr())
    ws = Region(_call(*args, None, what), dev)
    _call(*args, ws, what)
    assert T.same_bits(da.cpu(), da2.cpu()) and (db is None or T.same_bits(db.cpu(), db2.cpu())), f"{what}: dq | dk | dv differ"
    assert drel is None or T.same_bits(drel.cpu(), drel2.cpu()), f"{what}: d_rel differs"
    dq_, dk_, dv_ = (t.reshape(t.shape[0], c.B, c.H, c.hd).permute(1, 2, 0, 3).cpu() for t in _train.RelAttentionFn._split(da, db))
    _hold(r, route, T.AttnBwd(dq_, dk_, dv_, None if drel is None else drel.cpu()), refs, what + " through RelAttentionFn")
