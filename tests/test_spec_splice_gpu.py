"""isi_spec_splice_f32 and isi_spec_splice_blend_f32 (csrc/spec_splice.hip) against their float64 specification
(tests/spec_splice_spec.py, which also holds the data, the bound and the comparison), and the path above them:
SpectrogramsHelper.to_audio_spliced on helpers of n_fft 256 / hop 64 (plain and mel), inpainting.codes_to_audio_spliced and
the /get-audio-spliced route on the seeded small model of tests/test_code_mix_gpu.py.

Kernel cases: F in {1, 5, 64, 130} x T in {1, 2, 3, 17, 40} x B in {1, 3} x both w_batch forms x both mel values; the rows of a
case cycle through: no run, the whole row (w == 1 and fractional), a run at frame 0, a run ending at T, runs of one frame one
frame apart, several runs with fractional and whole weights, an interior run with ramps; silent original bins under
fractional weights; |psi| up to 40 pi.  Outputs sit inside poisoned buffers and the inputs are checked unchanged.

Figures of an MI355X run (profiles/spec_splice_checks.txt holds every case): the worst splice case reaches 0.575 of its
bound (B = 3, T = 40, F = 130, w_batch = 1, mel = 0) and the worst blend case 0.862 (n_fft 64, hop 32; the float32 numpy
model of the blend gives the same figure there).  End to end, rms inside the hole, locked against naive splice: plain helper
0.0287 against 0.9059, mel helper 0.0172 against 0.9571; with w == 1 everywhere the spliced call differs from `to_audio`,
where g == 1, by at most 2.3e-10 (plain) and 1.5e-8 (mel), far inside the bound derived in that test.

A recording aid, not a check: with ISI_SPEC_SPLICE_RECORD=<file> in the environment the worst error / bound ratio of every
kernel case is written there when the module ends."""
import io
import json
import math
import os

import numpy as np
import pytest
import torch

import spec_splice_spec as S

pytestmark = pytest.mark.gpu

RECORD = []      # (ratio, case name)
GUARD = 64       # floats of poison in front of and behind an output buffer
U = S.U


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_SPEC_SPLICE_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# worst error / bound of isi_spec_splice_f32 and isi_spec_splice_blend_f32 against the float64 spec, per case of\n"
                "# tests/test_spec_splice_gpu.py; the bound: tests/spec_splice_spec.py.  Worst first; copied elements and whole-row\n"
                "# runs at w == 1 are compared bit for bit in every case.\n")
        for ratio, what in sorted(RECORD, key=lambda r: -r[0]):
            f.write(f"{ratio:8.3f}  {what}\n")


def _poisoned(n, dev):
    buf = torch.full((GUARD + n + GUARD,), S.OUT_POISON, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _guards_clean(buf, n):
    host = buf.cpu()
    return bool((host[:GUARD] == S.OUT_POISON).all()) and bool((host[GUARD + n:] == S.OUT_POISON).all())


def _same_bits(t, array):
    return np.array_equal(S.bits(t.cpu().numpy()), S.bits(array))


# ------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("F", S.KERNEL_F)
@pytest.mark.parametrize("T", S.KERNEL_T)
def test_splice_kernel_against_the_spec(T, F):
    from interactive_spectrogram_inpainting import _hip
    L, dev = _hip.lib(), _dev()
    st = _hip.stream_ptr(dev)
    for case in S.kernel_cases(T, F):
        B = case.B
        xo, a, ph, w = (torch.from_numpy(x).to(dev) for x in (case.xo, case.a, case.ph, case.w))
        n = B * T * 2 * F
        buf, out = _poisoned(n, dev)
        rc = L.isi_spec_splice_f32(xo.data_ptr(), a.data_ptr(), ph.data_ptr(), w.data_ptr(), case.w_batch, out.data_ptr(), B, T, F,
                                   case.mel, st)
        assert rc == 0, L.isi_last_error()
        plain = torch.empty(B, T, 2 * F, device=dev)
        assert L.isi_spec_to_stft_f32(a.data_ptr(), ph.data_ptr(), plain.data_ptr(), B * T, F, case.mel, st) == 0
        torch.cuda.synchronize()
        assert _guards_clean(buf, n), f"{case.name}: a write outside the output"
        assert _same_bits(xo, case.xo) and _same_bits(a, case.a) and _same_bits(ph, case.ph) and _same_bits(w, case.w), \
            f"{case.name}: the kernel changed an input"
        got = out.cpu().numpy().reshape(B, T, 2 * F)
        ratio = S.compare(got, case, exact_ref=plain.cpu().numpy())
        print(f"{case.name}: worst error / bound = {ratio:.3f}")
        RECORD.append((ratio, "splice " + case.name))


@pytest.mark.parametrize("geometry", S.BLEND_GEOMETRIES)
def test_blend_kernel_against_the_spec(geometry):
    from interactive_spectrogram_inpainting import _hip
    L, dev = _hip.lib(), _dev()
    for B in (1, 3):
        case = S.make_blend_case(*geometry, B)
        orig, ola, touched = (torch.from_numpy(x).to(dev) for x in (case.orig, case.ola, case.touched))
        n = B * case.L
        buf, out = _poisoned(n, dev)
        rc = L.isi_spec_splice_blend_f32(orig.data_ptr(), ola.data_ptr(), touched.data_ptr(), out.data_ptr(), B, case.Tf, case.n_fft,
                                         case.hop, case.L, _hip.stream_ptr(dev))
        assert rc == 0, L.isi_last_error()
        torch.cuda.synchronize()
        assert _guards_clean(buf, n), f"{case.name}: a write outside the output"
        assert _same_bits(orig, case.orig) and _same_bits(ola, case.ola) and np.array_equal(touched.cpu().numpy(), case.touched)
        ratio = S.compare_blend(out.cpu().numpy().reshape(B, case.L), case)
        print(f"{case.name}: worst error / bound = {ratio:.3f}")
        RECORD.append((ratio, "blend " + case.name))


# ------------------------------------------------------------------------------------- end to end: to_audio_spliced
N_FFT, HOP, T_E2E = 256, 64, 64


class _EndToEnd:
    """one helper, two sounds (the experiment's three partials; partials plus noise), their spectrograms, the reference
    `to_audio` -- computed once"""

    def __init__(self, mel):
        from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper, SpectrogramsHelper
        cls = MelSpectrogramsHelper if mel else SpectrogramsHelper
        self.helper = cls(fs_hz=16000, n_fft=N_FFT, hop_length=HOP, window_length=N_FFT).to(_dev())
        self.signal = S.experiment_signal(T=T_E2E, n_fft=N_FFT, hop=HOP)
        g = np.random.default_rng(5)
        second = S.experiment_signal(T=T_E2E, n_fft=N_FFT, hop=HOP, seed=1).audio + 0.05 * g.standard_normal(T_E2E * HOP).astype(np.float32)
        self.audio_np = np.stack([self.signal.audio, second.astype(np.float32)])
        self.audio = torch.from_numpy(self.audio_np).to(_dev())
        self.spec = self.helper.to_spectrogram(self.audio)
        self.plain = self.helper.to_audio(self.spec)
        self.extra = N_FFT // HOP - 1

    def shares(self, touched_frames):
        """the blend's specification for frames [B, T] touched (the frames past T never are)"""
        touched = np.zeros((2, T_E2E + self.extra), dtype=np.uint8)
        touched[:, :T_E2E] = touched_frames
        return S.blend(self.audio_np, self.audio_np, touched, N_FFT, HOP)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "mel"])
def e2e(request):
    return _EndToEnd(request.param)


def test_weight_zero_returns_the_input_audio_bit_for_bit(e2e):
    for w_batch in (1, 2):
        w = torch.zeros(w_batch, T_E2E, N_FFT // 2, device=_dev())
        assert torch.equal(e2e.helper.to_audio_spliced(e2e.spec, e2e.audio, w), e2e.audio)


def test_weight_one_returns_to_audio_where_every_frame_is_regenerated(e2e):
    """The spliced STFT's first T frames are then `to_audio`'s own (whole-row runs at w == 1: isi_spec_to_stft_f32's bits), and
    where g == 1 the frames past T do not reach.  What may differ: the iSTFT GEMM runs on T + 3 rows per item instead of T (its
    tile route, hence its summation order, may change) and the blend computes orig + 1 (ola - orig).  Bound per sample, with
    mass = sum over the reaching frames and the 2F bins of |X| |basis|: two GEMMs of K = 2F split-f16 products (each operand in
    two 11-bit pieces, the lo x lo term dropped: below 2^-21 per product) accumulated in float32 ((K + 4) u, the overlap-add's
    four terms included), and the blend's two roundings u (2 |ola - orig| + |out|)."""
    helper, F = e2e.helper, N_FFT // 2
    w = torch.ones(1, T_E2E, F, device=_dev())
    got = helper.to_audio_spliced(e2e.spec, e2e.audio, w).cpu().numpy().astype(np.float64)
    want = e2e.plain.cpu().numpy().astype(np.float64)
    full = e2e.shares(1).full
    assert full[:, :(T_E2E - e2e.extra) * HOP].all() and not full[:, -1].any()
    _, (spec, a, ph) = helper._to_audio(e2e.spec, keep=True)
    X = np.abs(S.to_stft_f32_model(a.cpu().numpy(), ph.cpu().numpy(), int(helper.mel)).astype(np.float64))      # [B, T, 2F]
    basis = np.abs(helper._dft_bases()[1].numpy().astype(np.float64))                                            # [2F, n_fft]
    frames = X @ basis
    mass = np.zeros((2, T_E2E * HOP + N_FFT))
    for t in range(T_E2E):
        mass[:, t * HOP:t * HOP + N_FFT] += frames[:, t]
    mass = mass[:, N_FFT - HOP:N_FFT - HOP + T_E2E * HOP]
    orig = e2e.audio_np.astype(np.float64)
    bound = 2 * (2.0 ** -21 + (2 * F + 4) * U) * mass + U * (2 * np.abs(want - orig) + np.abs(want))
    err = np.abs(got - want)
    print(f"largest difference from to_audio where g == 1: {err[full].max():.3e}, largest error / bound {(err[full] / bound[full]).max():.3f}")
    assert (err[full] <= bound[full]).all()


def test_an_interior_hole_leaves_untouched_samples_bit_equal(e2e):
    F, dev = N_FFT // 2, _dev()
    w = torch.zeros(2, T_E2E, F, device=dev)
    w[0, 25:39] = 1.0                                    # every bin
    w[1, 10:12, 7:40] = 0.5                              # some bins, a fractional weight
    w[1, 50:51, 100] = 1.0
    got = e2e.helper.to_audio_spliced(e2e.spec, e2e.audio, w)
    touched = (w > 0).any(-1).cpu().numpy()
    s = e2e.shares(touched)
    assert s.copied.any() and (~s.copied).any()
    got_np = got.cpu().numpy()
    assert np.array_equal(S.bits(got_np)[s.copied], S.bits(e2e.audio_np)[s.copied])
    assert np.isfinite(got_np).all() and (got_np[~s.copied] != e2e.audio_np[~s.copied]).any()


def test_locked_splice_beats_the_naive_one(e2e):
    """The experiment of tests/test_spec_splice_host.py on the device: the decoded spectrogram is the original's own with 0.02 rad
    of jitter on the instantaneous frequency and a random start phase; 14 frames are regenerated.  The naive splice drops
    `to_audio`'s STFT frames into the original's.  rms difference from the original over the samples all of whose frames are
    regenerated; asserted: locked <= 0.1 naive."""
    from interactive_spectrogram_inpainting import _hip
    helper, dev, F, e = e2e.helper, _dev(), N_FFT // 2, e2e.signal
    L, st = _hip.lib(), _hip.stream_ptr(dev)
    g = torch.Generator().manual_seed(3)
    spec = e2e.spec[:1].clone()
    spec[0, 1] += (0.02 / math.pi) * torch.randn(F, T_E2E, generator=g).to(dev)
    spec[0, 1, :, 0] = (torch.rand(F, generator=g).to(dev) * 2 - 1)
    audio = e2e.audio[:1].contiguous()
    w = torch.from_numpy(e.w).to(dev)
    locked = helper.to_audio_spliced(spec, audio, w)[0].cpu().numpy()
    # the naive splice, from the same stages
    X_all, T_all = helper._stft(torch.nn.functional.pad(audio, (0, e2e.extra * HOP)))
    _, (_, a, ph) = helper._to_audio(spec, keep=True)
    X_dec = torch.empty(1, T_E2E, 2 * F, device=dev)
    assert L.isi_spec_to_stft_f32(a.data_ptr(), ph.data_ptr(), X_dec.data_ptr(), T_E2E, F, int(helper.mel), st) == 0
    X_naive = X_all.clone()
    X_naive[:, :T_E2E] = torch.where(torch.cat([w, w], -1) > 0, X_dec, X_all[:, :T_E2E])
    from interactive_spectrogram_inpainting.priors import _ops as gemm
    frames = gemm.linear(X_naive, helper._build(dev)["istft_w"], None, N_FFT)
    ola, naive = torch.empty(1, T_E2E * HOP, device=dev), torch.empty(1, T_E2E * HOP, device=dev)
    assert L.isi_overlap_add_f32(frames.data_ptr(), ola.data_ptr(), 1, T_all, N_FFT, HOP, N_FFT - HOP, T_E2E * HOP, st) == 0
    touched = torch.from_numpy(e.touched).to(dev)
    assert L.isi_spec_splice_blend_f32(audio.data_ptr(), ola.data_ptr(), touched.data_ptr(), naive.data_ptr(), 1, T_all, N_FFT, HOP,
                                       T_E2E * HOP, st) == 0
    torch.cuda.synchronize()
    rms_locked, rms_naive = S.experiment_rms(e, locked, naive[0].cpu().numpy())
    _, rms_plain = S.experiment_rms(e, locked, e2e.plain[0].cpu().numpy())
    print(f"rms inside the hole: locked {rms_locked:.4f}, naive {rms_naive:.4f}, ratio {rms_locked / rms_naive:.4f}; "
          f"to_audio of the original's own spectrogram, same samples: {rms_plain:.4f}")
    assert rms_locked <= 0.1 * rms_naive


# ------------------------------------------------------------------- codes_to_audio_spliced, the route: the small model
class _Model:
    """the seeded model of tests/test_code_mix_gpu.py, a helper whose spectrograms are its inputs' size ([2, 64, 128]), and
    an `upload` with its codes"""

    def __init__(self):
        import inpainting
        from GANsynth_pytorch.spectrograms_helper import SpectrogramsHelper
        from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
        from oracle import vqvae_oracle as O
        cfg = O.Config(in_channel=2)
        sd = O.init_state_dict(cfg, seed=4)
        O.calibrate_codebooks(sd, cfg, torch.randn(4, 2, 64, 128, generator=torch.Generator().manual_seed(9)))
        m = VQVAE(in_channel=2)
        m.load_state_dict(sd)
        self.m = m.to(_dev()).eval()
        self.K = cfg.num_embeddings
        self.helper = SpectrogramsHelper(fs_hz=16000, n_fft=128, hop_length=32, window_length=128).to(_dev())
        self.n = 128 * 32
        sound = S.experiment_signal(T=128, n_fft=128, hop=32, seed=2).audio
        self.audio = torch.from_numpy(0.4 * sound)
        self.top, self.bottom = inpainting.analyze_audio(self.m, self.helper, self.audio, self.n, _dev())

    def edited(self, columns=(5, 8)):
        top = self.top.clone()
        top[..., columns[0]:columns[1]] = (top[..., columns[0]:columns[1]] + 1) % self.K
        return top


@pytest.fixture(scope="module")
def model():
    return _Model()


def test_unchanged_codes_return_the_upload_bit_for_bit(model):
    import inpainting
    got = inpainting.codes_to_audio_spliced(model.m, model.helper, model.audio, model.top, model.bottom)
    assert got.shape == (1, model.n) and torch.equal(got[0].cpu(), model.audio)
    short = model.audio[:3000]                                           # trimmed / zero-padded as analyze_audio does
    top, bottom = inpainting.analyze_audio(model.m, model.helper, short, model.n, _dev())
    got = inpainting.codes_to_audio_spliced(model.m, model.helper, short, top, bottom)
    assert torch.equal(got[0, :3000].cpu(), short) and not got[0, 3000:].any()


def test_a_changed_window_leaves_the_samples_outside_its_support_bit_equal(model):
    import inpainting
    top = model.edited()
    got = inpainting.codes_to_audio_spliced(model.m, model.helper, model.audio, top, model.bottom)[0].cpu().numpy()
    mask = inpainting.changed_cells(model.top, model.bottom, top, model.bottom)
    assert mask[:, 5:8].all() and not mask[:, :5].any() and not mask[:, 8:].any()
    frames_per_column = 128 // model.top.shape[-1]
    weights = inpainting.splice_weights(model.helper, mask, 128, frames_per_column, halo_top=1)      # the defaults
    touched = np.zeros((1, 128 + 3), dtype=np.uint8)
    touched[0, :128] = (weights[0] > 0).any(-1).numpy()
    lo, hi = (5 - 1 - 1) * frames_per_column, (8 + 1 + 1) * frames_per_column                        # halo, then feather
    assert touched[0, lo + 1:hi - 1].all() and not touched[0, :lo].any() and not touched[0, hi:].any()
    audio = model.audio.numpy()[None]
    s = S.blend(audio, audio, touched, 128, 32)
    assert s.copied.mean() > 0.5
    assert np.array_equal(S.bits(got[None])[s.copied], S.bits(audio)[s.copied])
    assert np.isfinite(got).all() and (got[None][~s.copied] != audio[~s.copied]).any()
    with_mask = inpainting.codes_to_audio_spliced(model.m, model.helper, model.audio, top, model.bottom, mask_top=mask)
    assert np.array_equal(S.bits(with_mask[0].cpu().numpy()), S.bits(got))


def test_get_audio_spliced_route(model):
    import flask_server
    import inpainting
    app = flask_server.create_app(model.m, None, None, {}, _dev(), spectrograms_helper=model.helper)
    client = app.test_client()
    top = model.edited()
    codes = json.dumps({'top_code': top[0].tolist(), 'bottom_code': model.bottom[0].tolist()})
    wav = flask_server._wav_bytes(model.audio, 16000)
    upload, _ = flask_server._read_wav(wav)                               # what the route sees: 16-bit samples
    r = client.post('/get-audio-spliced', data={'audio': (io.BytesIO(wav), 'upload.wav'), 'codes': codes},
                    content_type='multipart/form-data')
    assert r.status_code == 200 and r.mimetype == "audio/wav"
    want = inpainting.codes_to_audio_spliced(model.m, model.helper, upload, top, model.bottom)[0]
    assert r.data == flask_server._wav_bytes(want, 16000)
    r = client.post('/get-audio-spliced?fs_hz=8000', data={'audio': (io.BytesIO(wav), 'upload.wav'),
                                                           'codes': (io.BytesIO(codes.encode()), 'codes.json')},
                    content_type='multipart/form-data')
    assert r.status_code == 200
    samples, rate = flask_server._read_wav(r.data)
    assert rate == 8000 and abs(samples.numel() - model.n // 2) <= 1
