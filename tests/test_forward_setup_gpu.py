"""Set-up of the forward that depends on the weights only, done once at pack time (csrc/vq_nearest.hip, vqvae_run.cpp):
the fused codebook searches copy the pack-time image of their LDS content (both f16 planes, the adjusted |e|^2, the
far-code words: isi_vq_pack_planes_f32) instead of deriving it in every workgroup of every launch, and the first encoder
launch zeroes both code histograms instead of a launch of its own.  ISI_NO_SETUP_FUSION restores the per-launch fill and
the zeroing launch; every test compares the two in one process, BITWISE.

The image against the in-kernel fill: the pack kernel RUNS the in-kernel fill (vq_fill_planes) and writes its LDS out,
so there is no second implementation to compare byte for byte; the tests below check the image's plain parts directly
(|e|^2 with its padding, far and poison marks, the far words) and everything else through the indices and the
e2-dependent outputs of forwards on codebooks with padded, far, non-finite and far-and-non-finite rows.

Shapes: the smallest that reach every branch -- a single work item per launch, partial tiles with fewer workgroups than
CUs, and one batch with more work items than workgroups."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

KNOB = "ISI_NO_SETUP_FUSION"
SHAPES = [(1, 2, 32, 64), (3, 2, 64, 144), (32, 2, 128, 512)]


def _hip():
    from interactive_spectrogram_inpainting import _hip as real
    return real


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _model(seed=4, precision="split_f16", **kw):
    from oracle import vqvae_oracle as O
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    cfg = O.Config(in_channel=2, **kw)
    sd = O.init_state_dict(cfg, seed=seed)
    g = torch.Generator().manual_seed(9)
    O.calibrate_codebooks(sd, cfg, torch.randn(2, 2, 64, 128, generator=g))
    m = VQVAE(in_channel=2, **kw)
    m.load_state_dict(sd)
    m.conv_precision = precision
    return m.to(_dev()).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


def _input(shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(_dev())


def _bits(t):
    """the tensor's bytes (NaN-safe equality: a poisoned search makes diff NaN on both paths)"""
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(got, ref, what):
    names = ("dec", "diff", "perplexity_t", "perplexity_b", "id_t", "id_b")
    for n, a, b in zip(names, got, ref):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: {n} differs from the per-launch set-up"


def _both(m, x):
    got = m(x)
    with _hip().knob(KNOB, 1):
        ref = m(x)
    return got, ref


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_packed_setup_equals_the_per_launch_one(model, shape):
    x = _input(shape)
    got, ref = _both(model, x)
    _assert_same(got, ref, f"input {shape}")
    assert torch.isfinite(got[1]).all() and float(got[2]) > 1.0 and float(got[3]) > 1.0
    enc = model.encode(x)                       # encode-only calls take the same tail
    with _hip().knob(KNOB, 1):
        enc_ref = model.encode(x)
    for a, b in zip(enc, enc_ref):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("precision", ["split_f16", "split_bf16"])
def test_both_precisions(precision):
    """split_f16 runs the fused searches; split_bf16 the two-launch quantiser, which the knob leaves alone"""
    m = _model(seed=5, precision=precision)
    for shape in SHAPES[:2]:
        got, ref = _both(m, _input(shape, seed=3))
        _assert_same(got, ref, f"{precision} {shape}")


def test_codebook_edge_rows():
    """K = 500 (histogram and planes padded to 512) with one code far outside the f16 planes' range (|e| >= 64)"""
    m = _model(seed=6, num_embeddings=500)
    with torch.no_grad():
        m.quantize_t.embed[:, 7] *= 400.0
        m.quantize_b.embed[:, 499] = 100.0
    for shape in SHAPES[:2]:
        got, ref = _both(m, _input(shape, seed=1))
        _assert_same(got, ref, f"K=500 {shape}")
        assert int(got[4].max()) < 500 and int(got[5].max()) < 500


def test_weights_overwritten_in_place():
    """the image lives and dies with the plan: new codebook / weights in place, the next forward is the new weights'"""
    m = _model(seed=7)
    x = _input(SHAPES[1], seed=2)
    before = m(x)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        e = m.quantize_t.embed
        e.copy_(e[:, torch.randperm(e.shape[1], generator=g).to(e.device)] * 1.25)
        w2 = m.enc_t.blocks[m.enc_t._res[0]].conv[3].weight
        w2.mul_(0.5)
    got, ref = _both(m, x)
    _assert_same(got, ref, "after the in-place update")
    assert not torch.equal(before[4], got[4]) or not torch.equal(before[0], got[0])


def _run_raw(m, x, fill, knob=0):
    """isi_vqvae_run through the C ABI on a caller-owned workspace pre-filled with `fill`"""
    H_ = _hip()
    L = H_.lib()
    B, _, H, W = x.shape
    Hb, Wb, Ht, Wt, Wq = m._latent_shapes(H, W)
    dev = x.device
    w = m._native_weights()
    nbytes = L.isi_vqvae_workspace_bytes(C.byref(w), B, H, W)
    assert nbytes > 0
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    id_t = torch.empty(B, Ht, Wt, dtype=torch.int64, device=dev)
    id_b = torch.empty(B, Hb, Wq, dtype=torch.int64, device=dev)
    scal = torch.full((5,), float("nan"), device=dev)
    dec = torch.empty(B, 2, Hb * 4, Wq * 4, device=dev)
    out = H_.isi_vqvae_out(dec.data_ptr(), None, None, id_t.data_ptr(), id_b.data_ptr(), scal.data_ptr())
    results = []
    for _ in range(2):                       # the SAME workspace twice, dirtied before each call
        ws.fill_(fill)
        with H_.knob(KNOB, knob):
            H_.check(L.isi_vqvae_run(C.byref(w), H_.MODE_FORWARD, x.data_ptr(), B, H, W, C.byref(out), ws.data_ptr(), nbytes,
                                     C.c_void_p(H_.stream_ptr(dev))), "isi_vqvae_run")
        torch.cuda.synchronize()
        results.append((dec.clone(), scal[4].reshape(1).clone(), scal[1].clone(), scal[3].clone(), id_t.clone(), id_b.clone()))
    return results


def _plan_tensor(m, ptr):
    return next(t for t in m._plan[1] if t.data_ptr() == ptr)


def test_image_rows_and_poisoned_codebook():
    """K = 500: rows 500..511 are padding (+2^100); a far row gets +2^100 and its bit in the far words, far[0] = the
    smallest |e|^2 of the far rows; a non-finite row -2^100, also where it is far as well.  Then forwards on that codebook
    (every top index -1, loud) through the C ABI: the Python layer would move such a model to split_bf16."""
    H_ = _hip()
    L = H_.lib()
    m = _model(seed=6, num_embeddings=500)
    with torch.no_grad():
        m.quantize_t.embed[:, 7] *= 400.0          # far
        m.quantize_t.embed[:, 40] *= 900.0         # far, and made non-finite below
    x = _input(SHAPES[1], seed=1)
    m(x)
    w = m._native_weights()
    codes, e2 = m.quantize_t.packed()               # the tensors the plan points at
    assert w.quantize_t.codes_kd == codes.data_ptr() and w.quantize_t.planes
    codes[11, 3] = float("inf"); e2[11] = float("inf")
    codes[40, 5] = float("nan"); e2[40] = float("nan")
    planes = _plan_tensor(m, w.quantize_t.planes)
    assert planes.numel() == L.isi_vq_planes_bytes(500) == 512 * 260 + 4 * 20
    H_.check(L.isi_vq_pack_planes_f32(codes.data_ptr(), e2.data_ptr(), planes.data_ptr(), 64, 500,
                                      C.c_void_p(H_.stream_ptr(codes.device))), "isi_vq_pack_planes_f32")
    img = planes.cpu()
    e2_img = img[512 * 256:512 * 260].view(torch.float32)
    far = img[512 * 260:].view(torch.int32)
    pad = 2.0 ** 100
    want = e2.cpu().clone()
    want[7] = pad; want[11] = -pad; want[40] = -pad
    assert torch.equal(e2_img[:500], want) and bool((e2_img[500:] == pad).all())
    assert far[0].view(torch.float32).item() == e2[7].item()
    bits = [int(v) & 0xFFFFFFFF for v in far[1:17]]
    assert bits[0] == 1 << 7 and not any(bits[1:]), "only the finite far row is marked"
    hi = img[:512 * 128].view(torch.int16).view(512, 64)
    assert not bool(hi[500:].any()) and bool(hi[0].any())
    ref = _run_raw(m, x, 0x00, knob=1)[0]
    got = _run_raw(m, x, 0xFF)[0]
    _assert_same(got, ref, "poisoned codebook")
    assert bool((got[4] == -1).all()) and bool(torch.isnan(got[1]).all())


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_dirty_workspace(model, shape):
    """the histograms are zeroed by the call itself: a workspace of 0xFF bytes, reused, changes nothing"""
    x = _input(shape, seed=5)
    with _hip().knob(KNOB, 1):
        ref = model(x)
    for k, got in enumerate(_run_raw(model, x, 0xFF)):
        _assert_same(got, ref, f"dirty workspace, call {k}")


def test_repeated_forwards_are_identical(model):
    x = _input(SHAPES[2], seed=8)
    with _hip().knob(KNOB, 1):
        ref = model(x)
    for k in range(20):
        got = model(x)
        for a, b in zip(got[1:4], ref[1:4]):
            assert torch.equal(_bits(a), _bits(b)), f"scalars of repetition {k}"
    _assert_same(got, ref, "20th repetition")
