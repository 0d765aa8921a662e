"""Code tables (csrc/code_tables.hip): dec_t's first 3x3 convolution and upsample_top_to_bottom[0] read nothing but the
quantised top map, so the plan carries their per-code products and one gather launch sums table rows instead of running
matrix work.  Specification: tests/code_tables_spec.py (float64).  ISI_NO_CODE_TABLES restores the convolutions.

Bounds.  A table entry is a double sum rounded to fp32 once: 2^-24 of its magnitude plus one ulp (the double sum's own
error, (D + 2) 2^-53 sum |w e| here and in the spec, is added: it matters only for an entry that cancels to nothing).
A gathered fp32 output adds the bias and at most nine rounded entries in fp32: 12 * 2^-24 * (|bias| + sum |terms|).  The
pair output is the fp32 output rounded to the pair format: 2^-23 of the maximum (tests/test_hip_parity.py's bound).
Against the convolution kernels (other summation order, split-f16 products): 2^-20 of the maximum.

Shapes: maps 1x1 (only the centre tap / one tap per phase inside), 1x3, 3x5 and 5x66 (crosses a wave's pixel group, a
workgroup's 8 / 16 columns and a 64-column boundary), B = 1 and 3."""
import ctypes

import pytest
import torch

import code_tables_spec as S

pytestmark = pytest.mark.gpu

KNOB = "ISI_NO_CODE_TABLES"
MAPS = [(1, 1), (1, 3), (3, 5), (5, 66)]
TOL = 1e-4


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _state(seed=4):
    from oracle import vqvae_oracle as O
    cfg = O.Config(in_channel=2)
    sd = O.init_state_dict(cfg, seed=seed)
    g = torch.Generator().manual_seed(9)
    O.calibrate_codebooks(sd, cfg, torch.randn(2, 2, 64, 128, generator=g))
    return cfg, sd


def _model_from(sd):
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    m = VQVAE(in_channel=2)
    m.load_state_dict(sd)
    return m.to(_dev()).eval()


class _Layers:
    """the two layers of a seeded default model, their GPU tables and the float64 spec tables (made once)"""

    def __init__(self):
        from interactive_spectrogram_inpainting.vqvae import _ops
        self.cfg, self.sd = _state()
        self.m = m = _model_from(self.sd)
        self.conv3, self.up = m.dec_t.blocks[0], m.upsample_top_to_bottom[0]
        self.codes, _ = m.quantize_t.packed()
        self.K, self.D = self.codes.shape
        self.C3, self.CU = self.conv3.out_channels, self.up.out_channels
        self.t3, self.tu = _ops.pack_code_tables(self.conv3.packed(), self.C3, self.up.packed(), self.CU, self.codes)
        w3, wT, e = self.conv3.weight.detach().cpu(), self.up.weight.detach().cpu(), self.codes.cpu()
        self.t3_spec, self.tu_spec = S.tables(w3, wT, e)
        self.t3_abs, self.tu_abs = S.tables(w3.abs(), wT.abs(), e.abs())
        self.b3, self.bU = self.conv3.bias.detach(), self.up.bias.detach()


@pytest.fixture(scope="module")
def layers():
    return _Layers()


def _ids(L, B, hw, seed=0):
    H, W = hw
    ids = torch.randint(0, L.K, (B, H, W), generator=torch.Generator().manual_seed(seed + 100 * H + W))
    ids[:, 0, 0], ids[:, -1, -1] = 0, L.K - 1                 # corners
    ids[:, 0, -1], ids[:, -1, 0] = L.K - 1, 0
    if W > 2:
        ids[:, 0, W // 2], ids[:, -1, W // 2] = L.K - 1, 0      # edges
    if H > 2:
        ids[:, H // 2, 0], ids[:, H // 2, -1] = 0, L.K - 1
    return ids


def _gather(L, ids, pair=False):
    from interactive_spectrogram_inpainting.vqvae import _ops
    o3, oU = _ops.code_gather(ids.to(_dev()), L.K, L.t3, L.b3, L.tu, L.bU, pair3=pair, pairU=pair)
    if pair:
        o3, oU = _ops.pair_decode(o3), _ops.pair_decode(oU)
    torch.cuda.synchronize()
    return o3.cpu(), oU.cpu()


def test_packed_tables_against_the_spec(layers):
    L = layers
    for got, spec, mag, rows in ((L.t3, L.t3_spec, L.t3_abs, 9 * L.K), (L.tu, L.tu_spec, L.tu_abs, 16 * L.K)):
        got = got.cpu()
        assert got.shape[0] == rows + 1
        pad = got[rows]
        assert bool((pad == 0).all()) and bool(torch.signbit(pad).all()), "the pad row is -0.0"
        spec, mag = spec.reshape(rows, -1), mag.reshape(rows, -1)
        ulp = torch.finfo(torch.float32).eps * 2.0 ** torch.floor(torch.log2(spec.abs().clamp(min=1e-300)))
        bound = 2.0 ** -24 * spec.abs() + ulp + 2 * (L.D + 2) * 2.0 ** -53 * mag
        err = (got[:rows].double() - spec).abs()
        print(f"table [{rows} x {got.shape[1]}]: worst error / bound = {(err / bound).max():.3f}")
        assert bool((err <= bound).all())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_gather_against_the_spec(layers, hw, B):
    L = layers
    ids = _ids(L, B, hw)
    got3, gotU = _gather(L, ids)
    ref3, mag3, _ = S.conv3_sum(L.t3_spec, L.b3.cpu(), ids, relu=True)
    refU, magU, _ = S.upsample_sum(L.tu_spec, L.bU.cpu(), ids)
    for name, got, ref, mag in (("conv3", got3, ref3, mag3), ("upsample", gotU, refU, magU)):
        assert got.shape == ref.shape
        err, bound = (got.double() - ref).abs(), 12 * 2.0 ** -24 * mag
        print(f"{name} {hw} B={B}: worst error / bound = {(err / bound).max():.3f}")
        assert bool((err <= bound).all()), name
    # the pair output is the fp32 output in the pair format
    pair3, pairU = _gather(L, ids, pair=True)
    for name, p, f in (("conv3", pair3, got3), ("upsample", pairU, gotU)):
        assert (p - f).abs().max() <= 2.0 ** -23 * f.abs().max(), name


@pytest.mark.parametrize("hw", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_gather_against_the_convolution_kernels(layers, hw):
    """the launches ISI_NO_CODE_TABLES restores, on the quantised map of the same ids (E[id] exactly; in the model the
    map also carries the straight-through rounding of z + (e - z))"""
    from interactive_spectrogram_inpainting.vqvae import _ops
    L = layers
    ids = _ids(L, 3, hw, seed=1)
    got3, gotU = _gather(L, ids)
    q = _ops.embed_code(ids.to(_dev()), L.codes).permute(0, 3, 1, 2)
    qp = _ops.pair_encode(q)
    old3 = _ops.conv2d(qp, L.conv3.packed(), L.b3, L.C3, 3, 1, 1, relu=True, bf16x3=4, extra_flags=_ops.PAIR_IN0)
    oldU = _ops.conv_transpose2d_k4s2(qp, L.up.packed(), L.bU, L.CU, relu=False, bf16x3=4, extra_flags=_ops.PAIR_IN0)
    for name, got, old in (("conv3", got3, old3), ("upsample", gotU, oldU)):
        old = old.permute(0, 2, 3, 1).cpu()
        err = (got - old).abs().max() / old.abs().max()
        print(f"{name} {hw}: table sum vs convolution kernel, max error / max = {err:.3e}")
        assert err <= 2.0 ** -20, name


@pytest.mark.parametrize("pair", [False, True], ids=["fp32", "pair"])
def test_bad_codes_are_loud(layers, pair):
    """a code outside [0, K) -- the search's -1 -- is NaN exactly on the pixels whose window contains it"""
    L = layers
    ids = _ids(L, 2, (5, 66), seed=2)
    ids[0, 2, 30] = -1            # interior
    ids[1, 0, 0] = -1             # corner
    ids[1, 4, 65] = L.K           # one past the codebook, the other corner
    got3, gotU = _gather(L, ids, pair=pair)
    _, _, bad3 = S.conv3_sum(L.t3_spec, L.b3.cpu(), ids)
    _, _, badU = S.upsample_sum(L.tu_spec, L.bU.cpu(), ids)
    for name, got, bad in (("conv3", got3, bad3), ("upsample", gotU, badU)):
        assert bad.any() and not bad.all()
        assert torch.equal(torch.isnan(got).all(-1), bad) and torch.equal(torch.isnan(got).any(-1), bad), name
        assert bool(torch.isfinite(got[~bad]).all()), name


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _x(shape=(3, 2, 64, 136), seed=12):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(_dev())


def test_whole_model_knob_on_and_off(layers):
    from interactive_spectrogram_inpainting import _hip
    from oracle import vqvae_oracle as O
    m, x = layers.m, _x()                                     # ragged width: cropped bottom grid
    w = m._native_weights()
    assert _hip.lib().isi_vqvae_pair_activations(ctypes.byref(w)) == 1 and w.code_table_conv3 and w.code_table_upsample
    got = m(x)
    with _hip.knob(KNOB, 1):
        ref = m(x)
    assert torch.equal(got[4], ref[4]), "no table feeds the top search"
    moved = (got[5] != ref[5]).float().mean().item()
    same = (got[5] == ref[5]).all(-1).all(-1)
    print(f"id_b differing between table and convolution path: {moved:.4%}; samples with equal ids: {int(same.sum())} of {len(same)}")
    assert moved < 0.01
    assert same.any(), "no sample left to compare"
    err = ((got[0][same] - ref[0][same]).abs().max() / ref[0][same].abs().max()).item()
    print(f"dec, table path vs convolution path: {err:.3e} of the maximum")
    assert err <= 3e-6
    oref = O.forward(x.cpu(), layers.sd, layers.cfg)
    agree = (got[4].cpu() == oref[4]).all(-1).all(-1) & (got[5].cpu() == oref[5]).all(-1).all(-1)
    if agree.any():
        err = ((got[0].cpu()[agree] - oref[0][agree]).abs().max() / oref[0][agree].abs().max()).item()
        print(f"dec against the oracle on {int(agree.sum())} samples with equal ids: {err:.3e}")
        assert err <= TOL
    forced = O.decode_code(got[4].cpu(), got[5].cpu(), layers.sd, layers.cfg)     # the decoder on the GPU's own codes
    err = ((got[0].cpu() - forced).abs().max() / forced.abs().max()).item()
    print(f"dec against the oracle's decoder on the same codes: {err:.3e}")
    assert err <= TOL


def test_forwards_repeat_and_do_not_depend_on_the_batch(layers):
    m, x = layers.m, _x(seed=13)
    a, b = m(x), m(x)
    assert _same(a, b)
    part = m(x[:2])
    assert torch.equal(_bits(part[0]), _bits(a[0][:2])) and torch.equal(part[4], a[4][:2]) and torch.equal(part[5], a[5][:2])
    enc = m.encode(x)                                          # encode() and forward() take the same route to id_b
    assert torch.equal(enc[3], a[4]) and torch.equal(enc[4], a[5])


def test_tables_follow_the_weights_and_the_codebook(layers):
    """in-place writes, load_state_dict and invalidate_plan rebuild the tables: the output is the new parameters'"""
    m = _model_from(layers.sd)
    x = _x(seed=14)
    before = m(x)
    with torch.no_grad():
        m.dec_t.blocks[0].weight.mul_(0.75)
    after_w = m(x)
    assert not torch.equal(before[0], after_w[0])
    assert _same(after_w, _model_from(m.state_dict())(x)), "in-place conv3 weight"
    k = int(after_w[4].flatten().mode().values)               # a top code in use
    with torch.no_grad():
        e = m.quantize_t.embed
        dup = (e == e[:, k:k + 1]).all(0)                     # the calibrated codebook tiles its samples: every copy of the row
        assert dup[k] and not dup.all()
        e[:, dup] = (e[:, int((~dup).nonzero()[0])] * 0.5).unsqueeze(1)
    after_e = m(x)
    assert not torch.equal(after_w[0], after_e[0])
    assert _same(after_e, _model_from(m.state_dict())(x)), "replaced codebook row"
    m.upsample_top_to_bottom[0].weight.data.mul_(1.25)        # through .data: no version bump
    m.invalidate_plan()
    after_i = m(x)
    assert not torch.equal(after_e[0], after_i[0])
    assert _same(after_i, _model_from(m.state_dict())(x)), "invalidate_plan"
    m.load_state_dict(layers.sd)
    assert _same(m(x), before), "load_state_dict"
