"""isi_formant_shift_f32 (csrc/formant.hip) against its float64 specification (tests/formant_spec.py, which also holds the data,
the derived bound and the comparison), and the path above it: GANsynth_pytorch.stretch.formant_shift / spectral_envelope /
shift_formants / transpose(preserve_formants=True) and bend.bend(preserve_formants=True) on helpers of n_fft 256 / hop 64
(plain and mel), inpainting.transpose_sound / bend_sound / shift_formants_sound and the routes /transpose-audio, /bend-audio
and /shift-formants on the seeded small model of tests/test_code_mix_gpu.py.

Kernel cases (formant_spec.kernel_cases): F in {2, 5, 64, 130, 1024} x T in {1, 3, 17} x every order of {2, 7, min(F, 64),
min(F, 256)}, with iterations in {1, 3, 16}, B in {1, 3} and both ratio_batch forms rotating through them, and F = 2048 with
order 256 once.  Frames cycle through a harmonic comb under an envelope, random bins, a silent frame, one loud bin, equal
magnitudes, a frame with a NaN, one with an infinity and a 200 dB dynamic range; ratio rows through all 1, constant up,
constant down, one value per frame, and 0, -1, 1e9, NaN, +-inf.  The output and the envelope sit inside poisoned buffers with
guards, the inputs are checked unchanged, copied frames are compared bit for bit.

A recording aid, not a check: with ISI_FORMANT_RECORD=<file> in the environment the worst error / bound ratio of every
kernel case and the end-to-end figures are written there when the module ends (profiles/formant_checks.txt is such a run)."""
import io
import os

import numpy as np
import pytest
import torch

import formant_spec as S
import stft_stretch_spec as R

pytestmark = pytest.mark.gpu

RECORD = []      # (ratio, case name)
NOTES = []       # end-to-end figures
GUARD = 64       # floats of poison in front of and behind an output buffer
U = S.U


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_FORMANT_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# worst error / bound of isi_formant_shift_f32 (output elements and envelope rows) against the float64 spec, per case\n"
                "# of tests/test_formant_gpu.py; the bound: tests/formant_spec.py.  Worst first; copied frames are compared bit for bit\n"
                "# in every case.  Behind them: the end-to-end figures.\n")
        for ratio, what in sorted(RECORD, key=lambda r: -r[0]):
            f.write(f"{ratio:8.4f}  {what}\n")
        for note in NOTES:
            f.write(f"# {note}\n")


def _note(text):
    print(text)
    NOTES.append(text)


def _same_bits(t, array):
    return np.array_equal(S.bits(t.cpu().numpy()), S.bits(array))


def _poisoned(n, dev):
    buf = torch.full((GUARD + n + GUARD,), S.OUT_POISON, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(torch.float32)


def _guards_intact(buf, n):
    host = buf.cpu()
    return bool((host[:GUARD] == S.OUT_POISON).all()) and bool((host[GUARD + n:] == S.OUT_POISON).all())


def _run_case(case, with_env=True):
    from interactive_spectrogram_inpainting import _hip
    L, dev = _hip.lib(), _dev()
    B, T, F = case.B, case.T, case.F
    Y, ratio, table = (torch.from_numpy(a).to(dev) for a in (case.Y, case.ratio, case.table))
    n, n_env = B * T * 2 * F, B * T * (F + 1)
    buf, out = _poisoned(n, dev)
    ebuf, env = _poisoned(n_env, dev)
    rc = L.isi_formant_shift_f32(Y.data_ptr(), ratio.data_ptr(), case.ratio_batch, table.data_ptr(), out.data_ptr(),
                                 env.data_ptr() if with_env else None, B, T, F, case.order, case.iterations, float(case.depth),
                                 float(case.max_gain), _hip.stream_ptr(dev))
    assert rc == 0, L.isi_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(buf, n) and _guards_intact(ebuf, n_env), f"{case.name}: a write outside an output"
    assert _same_bits(Y, case.Y) and _same_bits(ratio, case.ratio) and _same_bits(table, case.table), \
        f"{case.name}: the kernel changed an input"
    if not with_env:
        assert bool((ebuf == S.OUT_POISON).all()), f"{case.name}: the envelope was written without being asked for"
    return out.cpu().numpy().reshape(B, T, 2 * F), env.cpu().numpy().reshape(B, T, F + 1) if with_env else None


# ------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("F", S.KERNEL_F)
def test_kernel_against_the_spec(F):
    for i, case in enumerate(S.kernel_cases(F)):
        out, env = _run_case(case)
        ratio = S.compare(out, env, case)
        print(f"{case.name}: worst error / bound = {ratio:.4f}")
        RECORD.append((ratio, case.name))
        if i % 4 == 0:                                   # without the envelope: the same bits
            alone, _ = _run_case(case, with_env=False)
            assert np.array_equal(S.bits(alone), S.bits(out)), f"{case.name}: the output depends on env being asked for"


def test_the_cap_runs_and_a_frame_s_bits_depend_on_that_frame_alone():
    """F = 2048 with order 256 (two bins per lane of every loop); and frames of a batch, run alone with their own ratio, give
    the bits they gave in the batch"""
    case = S.flagship_case()
    out, env = _run_case(case)
    RECORD.append((S.compare(out, env, case), case.name))
    from GANsynth_pytorch.stretch import formant_shift
    dev = _dev()
    case = S.kernel_cases(130)[-1]                       # B = 3, T = 17, ratio_batch = 3
    Y, ratio = torch.from_numpy(case.Y).to(dev), torch.from_numpy(case.ratio).to(dev)
    whole, env = formant_shift(Y, ratio, case.order, case.iterations, return_envelope=True)
    for b, t in ((0, 0), (1, 5), (2, 16)):
        one, one_env = formant_shift(Y[b:b + 1, t:t + 1], ratio[b:b + 1, t:t + 1], case.order, case.iterations, return_envelope=True)
        assert _same_bits(one[0, 0], whole[b, t].cpu().numpy()) and _same_bits(one_env[0, 0], env[b, t].cpu().numpy())
    with pytest.raises(ValueError):
        formant_shift(torch.zeros(1, 2, 4098, device=dev), torch.ones(2, device=dev), 18)               # above the cap


# ------------------------------------------------------------------------------------- end to end: the formant tone
N_FFT, HOP, T_E2E, FS, F0 = 256, 64, 64, 16000, 440.0
ORDER = 18
SCALE = 0.1
EPS_I = 2 * (2.0 ** -21 + (N_FFT + 5) * U)            # the synthesis GEMM, as tests/test_stft_stretch_gpu.py derives it


def _overlap(frames):
    T = frames.shape[0]
    out = np.zeros(T * HOP + N_FFT)
    for t in range(T):
        out[t * HOP:t * HOP + N_FFT] += frames[t]
    return out[N_FFT - HOP:N_FFT - HOP + T * HOP]


class _EndToEnd:
    """one helper and the experiment's tone: all harmonics of 440 Hz under the fixed formant envelope, 64 frames"""

    def __init__(self, mel):
        from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper, SpectrogramsHelper
        cls = MelSpectrogramsHelper if mel else SpectrogramsHelper
        self.mel = mel
        self.name = "mel" if mel else "plain"
        self.helper = cls(fs_hz=FS, n_fft=N_FFT, hop_length=HOP, window_length=N_FFT).to(_dev())
        self.audio_np = (SCALE * S.formant_tone(T_E2E * HOP, F0, FS)).astype(np.float32)
        self.audio = torch.from_numpy(self.audio_np).to(_dev())
        _, inv = self.helper._dft_bases()
        self.inv = inv.numpy().astype(np.float64)                                              # [2F, n_fft]
        self.extra = N_FFT // HOP - 1
        self.plain = {}

    def plain_error(self, semitones):
        """the partial-amplitude error of the plain `transpose`, once per shift"""
        from GANsynth_pytorch.stretch import transpose, transpose_ratio
        if semitones not in self.plain:
            num, den, _ = transpose_ratio(semitones)
            y = transpose(self.helper, self.audio, semitones)
            self.plain[semitones] = (y, S.partial_error(y.cpu().numpy() / SCALE, F0, num / den, FS))
        return self.plain[semitones]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "mel"])
def e2e(request):
    return _EndToEnd(request.param)


@pytest.mark.parametrize("semitones", [3, -4, 7])
def test_transpose_with_formants_kept(e2e, semitones):
    """(1) Up to the resampler, the corrected stretch agrees with the float64 specification run on the device's own stretched
    frames (P, the copy rule and the interpolation cell are properties of those float32 bits): the kernel's bound per bin
    pushed through the synthesis basis, plus the synthesis' own error.  (2) The partial-amplitude error against E at the new
    partial frequencies is at most 0.7 of the plain transposition's.  (3) The pitch is where the plain transposition puts it.
    (4) A batch gives the same bits per row."""
    from GANsynth_pytorch.pitch import estimate_pitch
    from GANsynth_pytorch.stretch import stft_stretch, stretch_positions, time_stretch, transpose, transpose_ratio
    helper, dev = e2e.helper, _dev()
    num, den, _ = transpose_ratio(semitones)
    rho = num / den
    got = time_stretch(helper, e2e.audio, rho, _formant=(rho, ORDER)).cpu().numpy().astype(np.float64)
    X, T_all = helper._stft(torch.nn.functional.pad(e2e.audio[None], (0, e2e.extra * HOP)))
    pos = torch.cat([stretch_positions(T_E2E, factor=rho), torch.arange(T_E2E, T_all, dtype=torch.float32)])
    T_out = pos.numel() - e2e.extra
    Y = stft_stretch(X, pos.to(dev), HOP).cpu().numpy()
    spec = S.spec(Y, np.full((1, Y.shape[1]), rho, np.float32), ORDER, 16)
    F = N_FFT // 2
    Z = spec.out[0, :, :F] + 1j * spec.out[0, :, F:]
    want = R.istft(Z, N_FFT, HOP, T_out * HOP)
    inv_c, inv_s = np.abs(e2e.inv[:F]), np.abs(e2e.inv[F:])
    frames = EPS_I * (np.abs(Z.real) @ inv_c + np.abs(Z.imag) @ inv_s) + spec.bound[0, :, :F] @ inv_c + spec.bound[0, :, F:] @ inv_s
    bound = _overlap(frames)[:T_out * HOP] + U * np.abs(want)
    err = np.abs(got - want)
    assert got.shape == want.shape and (err <= bound).all(), f"error / bound = {(err / bound).max():.3f}"

    y = transpose(helper, e2e.audio, semitones, preserve_formants=True, formant_order=ORDER)
    assert y.shape == e2e.audio.shape and bool(torch.isfinite(y).all())
    plain_y, plain = e2e.plain_error(semitones)
    corrected = S.partial_error(y.cpu().numpy() / SCALE, F0, rho, FS)
    midi = float(estimate_pitch(y, FS)[0])
    _note(f"transpose({semitones:+d}, preserve_formants=True), {e2e.name} helper: partial amplitudes against E(rho h f0) "
          f"{corrected[0]:.2f} dB rms (largest {corrected[1]:.2f}), plain transpose {plain[0]:.2f} ({plain[1]:.2f}), ratio "
          f"{corrected[0] / plain[0]:.2f}; estimated pitch {midi:.4f}; stretched audio against the float64 spec: largest difference "
          f"{err.max():.3e}, largest error / bound {(err / bound).max():.4f}")
    assert corrected[0] <= 0.7 * plain[0]
    assert abs(midi - (69 + semitones)) <= 0.05
    assert not torch.equal(y, plain_y)
    both = transpose(helper, torch.stack([e2e.audio, e2e.audio]), semitones, preserve_formants=True, formant_order=ORDER)
    assert torch.equal(both[0], y) and torch.equal(both[1], y)


def test_the_default_path_is_untouched_and_the_order_is_found(e2e):
    """without the new arguments, and with preserve_formants=False, the same bits; the order from `pitch` and from the
    estimate of the sound is the explicit one's"""
    from GANsynth_pytorch.bend import bend
    from GANsynth_pytorch.stretch import transpose
    helper = e2e.helper
    plain_y, _ = e2e.plain_error(3)
    assert torch.equal(transpose(helper, e2e.audio, 3, preserve_formants=False), plain_y)
    both = transpose(helper, torch.stack([e2e.audio, e2e.audio]), 3, preserve_formants=False)
    assert torch.equal(both[0], plain_y) and torch.equal(both[1], plain_y)
    assert torch.equal(bend(helper, e2e.audio, 3.0), bend(helper, e2e.audio, 3.0, preserve_formants=False))
    explicit = transpose(helper, e2e.audio, 3, preserve_formants=True, formant_order=ORDER)
    assert torch.equal(transpose(helper, e2e.audio, 3, preserve_formants=True, pitch=69.0), explicit)
    assert torch.equal(transpose(helper, e2e.audio, 3, preserve_formants=True), explicit)            # the estimate: 440 Hz -> 18
    noise = 0.1 * torch.randn(T_E2E * HOP, generator=torch.Generator().manual_seed(1)).to(_dev())
    assert torch.equal(transpose(helper, noise, 3, preserve_formants=True),
                       transpose(helper, noise, 3, preserve_formants=True, formant_order=32))        # unvoiced: 32


def test_shift_formants_keeps_the_pitch_and_moves_the_envelope(e2e):
    """+4 semitones: the pitch stays, and the result's envelope (`spectral_envelope`) at bin k is the source's at k / 2^(4/12):
    closer to the moved source envelope than to the unmoved one.  The figures are recorded."""
    from GANsynth_pytorch.pitch import estimate_pitch
    from GANsynth_pytorch.stretch import shift_formants, spectral_envelope
    helper = e2e.helper
    assert shift_formants(helper, e2e.audio, 0) is e2e.audio
    y = shift_formants(helper, e2e.audio, 4.0, order=ORDER)
    assert y.shape == e2e.audio.shape and bool(torch.isfinite(y).all())
    midi = float(estimate_pitch(y, FS)[0])
    src = spectral_envelope(helper, e2e.audio, order=ORDER).cpu().numpy().astype(np.float64)
    res = spectral_envelope(helper, y, order=ORDER).cpu().numpy().astype(np.float64)
    F = N_FFT // 2
    assert src.shape == (T_E2E, F + 1) and res.shape == src.shape
    up = 2.0 ** (4.0 / 12.0)
    k = np.arange(8, int(0.9 * F))                                                 # away from DC and from Nyquist
    frames = slice(T_E2E // 4, 3 * T_E2E // 4)
    x = k / up
    i = np.floor(x).astype(int)
    moved = (1 - (x - i)) * src[frames][:, i] + (x - i) * src[frames][:, i + 1]
    rms = lambda d: float(np.sqrt(np.mean(d ** 2)) / S.DB)                          # noqa: E731
    to_moved, to_unmoved = rms(res[frames][:, k] - moved), rms(res[frames][:, k] - src[frames][:, k])
    _note(f"shift_formants(+4), {e2e.name} helper: estimated pitch {midi:.4f}; the result's envelope against the source's moved "
          f"{to_moved:.2f} dB rms, against the source's unmoved {to_unmoved:.2f}")
    assert abs(midi - 69.0) <= 0.05
    assert to_moved < to_unmoved
    both = shift_formants(helper, torch.stack([e2e.audio, e2e.audio]), 4.0, order=ORDER)
    assert torch.equal(both[0], y) and torch.equal(both[1], y)
    batch_env = spectral_envelope(helper, torch.stack([e2e.audio, e2e.audio]), pitch=69.0)
    assert batch_env.shape == (2, T_E2E, F + 1) and _same_bits(batch_env[1], src.astype(np.float32))


def test_bend_by_a_constant_agrees_with_transpose(e2e):
    """a constant curve of +3 with preserve_formants against transpose(+3, preserve_formants=True): the two differ by their
    resamplers (and the transposition's rational ratio); asserted is the partial-amplitude criterion, the difference is recorded"""
    from GANsynth_pytorch.bend import bend
    from GANsynth_pytorch.stretch import transpose, transpose_ratio
    helper = e2e.helper
    num, den, _ = transpose_ratio(3)
    bent = bend(helper, e2e.audio, 3.0, preserve_formants=True, formant_order=ORDER)
    assert bent.shape == e2e.audio.shape and bool(torch.isfinite(bent).all())
    moved = transpose(helper, e2e.audio, 3, preserve_formants=True, formant_order=ORDER)
    _, plain = e2e.plain_error(3)
    corrected = S.partial_error(bent.cpu().numpy() / SCALE, F0, 2.0 ** 0.25, FS)
    L = T_E2E * HOP
    mid = slice(L // 4, 3 * L // 4)
    diff = float((bent - moved)[mid].abs().max() / moved[mid].abs().max())
    _note(f"bend(+3 constant, preserve_formants=True), {e2e.name} helper: partial amplitudes {corrected[0]:.2f} dB rms (largest "
          f"{corrected[1]:.2f}) against the plain transpose's {plain[0]:.2f}; largest difference from transpose(+3, "
          f"preserve_formants=True) in the steady half, relative to its peak: {diff:.3e}")
    assert corrected[0] <= 0.7 * plain[0]
    assert not torch.equal(bent, bend(helper, e2e.audio, 3.0))
    assert torch.equal(bend(helper, e2e.audio, 3.0, preserve_formants=True, pitch=69.0), bent)


# ------------------------------------------------------------------------------------ the sounds and the routes: the small model
class _Model:
    """the seeded model of tests/test_code_mix_gpu.py, a helper whose spectrograms are its inputs' size ([2, 64, 128]), and a
    voiced sound"""

    def __init__(self):
        from GANsynth_pytorch.spectrograms_helper import SpectrogramsHelper
        from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
        from oracle import vqvae_oracle as O
        cfg = O.Config(in_channel=2)
        sd = O.init_state_dict(cfg, seed=4)
        O.calibrate_codebooks(sd, cfg, torch.randn(4, 2, 64, 128, generator=torch.Generator().manual_seed(9)))
        m = VQVAE(in_channel=2)
        m.load_state_dict(sd)
        self.m = m.to(_dev()).eval()
        self.helper = SpectrogramsHelper(fs_hz=16000, n_fft=128, hop_length=32, window_length=128).to(_dev())
        self.n = 128 * 32
        self.audio = torch.from_numpy((0.05 * S.formant_tone(self.n, 880.0)).astype(np.float32))


@pytest.fixture(scope="module")
def model():
    return _Model()


def test_sounds(model):
    import inpainting
    from GANsynth_pytorch import bend, stretch
    from GANsynth_pytorch.pitch import estimate_pitch
    dev = _dev()
    x = model.audio.to(dev)
    own = float(estimate_pitch(x, 16000)[0])
    y, top, bottom = inpainting.transpose_sound(model.m, model.helper, model.audio, to_pitch=own + 3.0, preserve_formants=True)
    assert torch.equal(y, stretch.transpose(model.helper, x, 3.0, preserve_formants=True, pitch=own))
    again = inpainting.analyze_audio(model.m, model.helper, y, model.n, dev)
    assert y.shape == (model.n,) and torch.equal(top, again[0]) and torch.equal(bottom, again[1])
    plain = inpainting.transpose_sound(model.m, model.helper, model.audio, to_pitch=own + 3.0, re_encode=False)[0]
    assert torch.equal(plain, stretch.transpose(model.helper, x, 3.0)) and not torch.equal(plain, y)
    got = float(estimate_pitch(y, 16000)[0])
    _note(f"transpose_sound(to_pitch = own + 3, preserve_formants=True): source {own:.3f}, result {got:.3f}")
    assert abs(got - own - 3.0) < 0.5
    by = inpainting.transpose_sound(model.m, model.helper, model.audio, semitones=-2.0, re_encode=False, preserve_formants=True)
    assert torch.equal(by[0], stretch.transpose(model.helper, x, -2.0, preserve_formants=True)) and by[1] is None

    g, top, bottom = inpainting.bend_sound(model.m, model.helper, model.audio, glide=(0.0, 2.0), preserve_formants=True)
    assert torch.equal(g, bend.glide(model.helper, x, 0.0, 2.0, preserve_formants=True)) and top is not None
    assert not torch.equal(g, inpainting.bend_sound(model.m, model.helper, model.audio, glide=(0.0, 2.0), re_encode=False)[0])
    flat = inpainting.bend_sound(model.m, model.helper, model.audio, flatten=True, to_pitch=own + 1.0, re_encode=False,
                                 preserve_formants=True)[0]
    assert flat.shape == (model.n,) and bool(torch.isfinite(flat).all())
    assert abs(float(estimate_pitch(flat, 16000)[0]) - own - 1.0) < 0.5

    s, top, bottom = inpainting.shift_formants_sound(model.m, model.helper, model.audio, 4.0)
    assert torch.equal(s, stretch.shift_formants(model.helper, x, 4.0))
    again = inpainting.analyze_audio(model.m, model.helper, s, model.n, dev)
    assert torch.equal(top, again[0]) and torch.equal(bottom, again[1])
    assert abs(float(estimate_pitch(s, 16000)[0]) - own) < 0.1
    same = inpainting.shift_formants_sound(model.m, model.helper, model.audio, 0.0, re_encode=False)
    assert torch.equal(same[0], x) and same[1] is None


def test_routes(model):
    import flask_server
    import inpainting
    app = flask_server.create_app(model.m, None, None, {}, _dev(), spectrograms_helper=model.helper)
    client = app.test_client()
    wav = flask_server._wav_bytes(model.audio, 16000)
    upload, _ = flask_server._read_wav(wav)                               # what the routes see: 16-bit samples
    post = lambda url, **form: client.post(url, data=dict(audio=(io.BytesIO(wav), 'upload.wav'), **form),      # noqa: E731
                                           content_type='multipart/form-data')
    r = post('/transpose-audio?semitones=3&preserve_formants=1')
    assert r.status_code == 200 and r.mimetype == "audio/wav"
    want = inpainting.transpose_sound(model.m, model.helper, upload, semitones=3.0, re_encode=False, preserve_formants=True)[0]
    assert r.data == flask_server._wav_bytes(want, 16000)
    plain = post('/transpose-audio?semitones=3')
    assert plain.status_code == 200 and plain.data != r.data
    assert post('/transpose-audio?semitones=3&preserve_formants=0').data == plain.data
    r = post('/bend-audio?glide_from=0&glide_to=2', preserve_formants='1')            # a form field
    assert r.status_code == 200
    want = inpainting.bend_sound(model.m, model.helper, upload, glide=(0.0, 2.0), re_encode=False, preserve_formants=True)[0]
    assert r.data == flask_server._wav_bytes(want, 16000)
    assert post('/bend-audio?glide_from=0&glide_to=2').data != r.data
    r = post('/shift-formants?semitones=4')
    assert r.status_code == 200 and r.mimetype == "audio/wav"
    want = inpainting.shift_formants_sound(model.m, model.helper, upload, 4.0, re_encode=False)[0]
    assert r.data == flask_server._wav_bytes(want, 16000)
    samples, rate = flask_server._read_wav(r.data)
    assert rate == 16000 and samples.numel() == model.n
    assert post('/shift-formants', semitones='-2.5').status_code == 200
    assert post('/shift-formants?semitones=40').status_code == 400
