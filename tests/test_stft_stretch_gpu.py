"""isi_stft_stretch_f32 (csrc/stft_stretch.hip) against its float64 specification (tests/stft_stretch_spec.py, which also holds
the data, the bound and the comparison), and the path above it: GANsynth_pytorch.stretch.time_stretch / transpose and
SpectrogramsHelper.to_audio_stretched on helpers of n_fft 256 / hop 64 (plain and mel), inpainting.stretch_sound /
transpose_sound and the routes /stretch-audio and /transpose-audio on the seeded small model of tests/test_code_mix_gpu.py.

Kernel cases: F in {1, 2, 5, 64, 130, 1024} x T in {2, 3, 17, 40} x T_out in {1, 2, T, 2T + 1} x B in {1, 3} x both pos_batch
forms.  Frames cycle through random bins, silent frames, equal magnitudes, a peak that moves one bin per frame, peaks at
bins 0 and F - 1 and a plateau of equal loud bins; rows of positions through a uniform stretch (copy run 1), rate 1 (copy
run min(T, T_out)), a fractional start (copy run 0), a frozen frame, decreasing positions, positions below 0, above T - 1,
NaN and infinite, random positions, and a copy run from frame 1.  The output sits inside a poisoned buffer, the inputs are
checked unchanged, `near` is read from the workspace and compared exactly.

Figures of an MI355X run (profiles/stft_stretch_checks.txt holds every case): the worst kernel case reaches 0.320 of its
bound (B = 3, T = 17, F = 1024, T_out = 2, pos_batch = 3).  End to end: time_stretch(factor = 1) differs from the float64
analysis + synthesis by at most 2.5e-7; at factors 1.5 / 2 the audio differs from the float64 specification's by at most
2.1e-6 / 2.7e-6 (0.008 / 0.009 of the bound) and its spectral convergence against the ideally stretched sound is 0.0475 /
0.0627; transpose by +3 / -4 semitones is estimated at 71.9997 / 65.0001; to_audio_stretched at rate 1 equals to_audio.

A recording aid, not a check: with ISI_STFT_STRETCH_RECORD=<file> in the environment the worst error / bound ratio of every
kernel case and the end-to-end figures are written there when the module ends."""
import io
import math
import os

import numpy as np
import pytest
import torch

import stft_stretch_spec as S

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
    path = os.environ.get("ISI_STFT_STRETCH_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# worst error / bound of isi_stft_stretch_f32 against the float64 spec, per case of tests/test_stft_stretch_gpu.py;\n"
                "# the bound: tests/stft_stretch_spec.py.  Worst first; copied frames are compared bit for bit and `near` exactly in\n"
                "# every case.  Behind them: the end-to-end figures.\n")
        for ratio, what in sorted(RECORD, key=lambda r: -r[0]):
            f.write(f"{ratio:8.3f}  {what}\n")
        for note in NOTES:
            f.write(f"# {note}\n")


def _note(text):
    print(text)
    NOTES.append(text)


def _same_bits(t, array):
    return np.array_equal(S.bits(t.cpu().numpy()), S.bits(array))


# ------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("F", S.KERNEL_F)
@pytest.mark.parametrize("T", S.KERNEL_T)
def test_kernel_against_the_spec(T, F):
    from interactive_spectrogram_inpainting import _hip
    L, dev = _hip.lib(), _dev()
    st = _hip.stream_ptr(dev)
    for case in S.kernel_cases(T, F):
        B, T_out = case.B, case.T_out
        X, pos = torch.from_numpy(case.X).to(dev), torch.from_numpy(case.pos).to(dev)
        n = B * T_out * 2 * F
        buf = torch.full((GUARD + n + GUARD,), S.OUT_POISON, dtype=torch.int32, device=dev)
        out = buf[GUARD:GUARD + n].view(torch.float32)
        need = L.isi_stft_stretch_workspace_bytes(B, T, F)
        assert need == 16 * B * T * F
        ws = torch.full((need // 4 + GUARD,), S.OUT_POISON, dtype=torch.int32, device=dev)
        rc = L.isi_stft_stretch_f32(X.data_ptr(), pos.data_ptr(), case.pos_batch, out.data_ptr(), ws.data_ptr(), need, B, T, T_out,
                                    F, case.hop, st)
        assert rc == 0, L.isi_last_error()
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[:GUARD] == S.OUT_POISON).all()) and bool((host[GUARD + n:] == S.OUT_POISON).all()), \
            f"{case.name}: a write outside the output"
        ws_host = ws.cpu().numpy()
        assert (ws_host[need // 4:] == S.OUT_POISON).all(), f"{case.name}: a write outside the workspace"
        assert _same_bits(X, case.X) and _same_bits(pos, case.pos), f"{case.name}: the kernel changed an input"
        near = ws_host[3 * B * T * F:4 * B * T * F].reshape(B, T, F)
        assert np.array_equal(near, case.spec.src.near), f"{case.name}: a peak decision differs"
        got = out.cpu().numpy().reshape(B, T_out, 2 * F)
        ratio = S.compare(got, case)
        print(f"{case.name}: worst error / bound = {ratio:.3f}")
        RECORD.append((ratio, case.name))


def test_flagship_size_rate_one_is_the_identity_bit_for_bit():
    """F = 1024, T = 125 (the flagship front-end), B = 2: pos = 0 .. T - 1 returns X; and F at the cap runs"""
    from GANsynth_pytorch.stretch import stft_stretch, stretch_positions
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    X = torch.randn(2, 125, 2048, generator=g).to(dev)
    assert torch.equal(stft_stretch(X, stretch_positions(125, factor=1).to(dev), 512), X)
    Y = stft_stretch(X, stretch_positions(125, factor=2.0).to(dev), 512)
    assert Y.shape == (2, 250, 2048) and bool(torch.isfinite(Y).all()) and torch.equal(Y[:, 0], X[:, 0])
    Xc = torch.randn(1, 5, 4096, generator=g).to(dev)                                   # F = 2048: two bins per lane
    assert torch.equal(stft_stretch(Xc, torch.arange(5.0, device=dev), 1024), Xc)
    source = S.make_source(1, 5, 2048)
    case = S.make_case(source, 9, 1)
    got = stft_stretch(torch.from_numpy(case.X).to(dev), torch.from_numpy(case.pos).to(dev), case.hop).cpu().numpy()
    RECORD.append((S.compare(got, case), case.name))
    with pytest.raises(ValueError):
        stft_stretch(torch.zeros(1, 5, 4098, device=dev), torch.arange(5.0, device=dev), 1)          # above the cap


# ---------------------------------------------------------------------------- end to end: time_stretch, transpose
N_FFT, HOP, T_E2E, FS = 256, 64, 64, 16000
EPS_F = 2 * (2.0 ** -21 + (N_FFT + 5) * U)            # the analysis convolution: K = n_fft products, see _synthesis_error
EPS_I = 2 * (2.0 ** -21 + (N_FFT + 5) * U)            # the synthesis GEMM: K = 2F = n_fft products


def _overlap(frames):
    """[T, n_fft] -> [T hop]: the helper's overlap-add of per-frame quantities"""
    T = frames.shape[0]
    out = np.zeros(T * HOP + N_FFT)
    for t in range(T):
        out[t * HOP:t * HOP + N_FFT] += frames[t]
    return out[N_FFT - HOP:N_FFT - HOP + T * HOP]


class _EndToEnd:
    """one helper, the experiment's sound (three decaying partials of 440 Hz, a 10 ms attack) with a little noise -- the
    float32 bits every test starts from"""

    def __init__(self, mel):
        from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper, SpectrogramsHelper
        cls = MelSpectrogramsHelper if mel else SpectrogramsHelper
        self.mel = mel
        self.helper = cls(fs_hz=FS, n_fft=N_FFT, hop_length=HOP, window_length=N_FFT).to(_dev())
        g = np.random.default_rng(5)
        self.audio_np = (0.5 * S.tone(T_E2E * HOP, 440.0) + 1e-3 * g.standard_normal(T_E2E * HOP)).astype(np.float32)
        self.audio = torch.from_numpy(self.audio_np).to(_dev())
        fwd, inv = self.helper._dft_bases()
        self.fwd, self.inv = np.abs(fwd.numpy().astype(np.float64)), inv.numpy().astype(np.float64)        # [2F, n_fft] each
        self.extra = N_FFT // HOP - 1


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "mel"])
def e2e(request):
    return _EndToEnd(request.param)


def _synthesis_error(e, Y, bound=None):
    """per sample: what the synthesis GEMM and the overlap-add may add to frames Y complex [T, F] (EPS_I times the mass of
    |Y| |basis|: split-f16 products, each operand in two 11-bit pieces with the lo x lo term dropped, below 2^-21 per product,
    float32 accumulation of K + 4 terms with the overlap-add's, the basis' own rounding, twice over as in
    tests/test_spec_splice_gpu.py), plus an error of at most `bound` [T, F] per complex bin pushed through the basis"""
    F = N_FFT // 2
    inv_c, inv_s = np.abs(e.inv[:F]), np.abs(e.inv[F:])
    frames = EPS_I * (np.abs(Y.real) @ inv_c + np.abs(Y.imag) @ inv_s)
    if bound is not None:
        frames = frames + bound @ np.hypot(e.inv[:F], e.inv[F:])
    return _overlap(frames)


def test_factor_one_returns_the_input(e2e):
    """time_stretch(factor = 1): every position is a whole frame in order, the STFT is copied bit for bit, and the result is
    the helper's analysis followed by its synthesis.  That pair drops the DC bin; the float64 pair of the specification does
    the same, so what it loses of this (nearly zero-mean) sound is known exactly and is added to the bound against the input.
    Bound: the analysis error, EPS_F times the
    mass of |x| |window basis| per bin, pushed through the synthesis basis, plus the synthesis' own (`_synthesis_error`)."""
    from GANsynth_pytorch.stretch import time_stretch
    got = time_stretch(e2e.helper, e2e.audio, 1.0).cpu().numpy().astype(np.float64)
    x = e2e.audio_np.astype(np.float64)
    T_all = T_E2E + e2e.extra
    X = S.stft(x, N_FFT, HOP, T_all)
    want = S.istft(X, N_FFT, HOP, T_E2E * HOP)
    xp = np.zeros((T_all - 1) * HOP + N_FFT)
    xp[N_FFT - HOP:N_FFT - HOP + len(x)] = np.abs(x)
    frames = np.stack([xp[t * HOP:t * HOP + N_FFT] for t in range(T_all)])
    mass = frames @ e2e.fwd.T                                                           # [T_all, 2F]
    F = N_FFT // 2
    bound = _synthesis_error(e2e, X, EPS_F * np.hypot(mass[:, :F], mass[:, F:]))[:T_E2E * HOP] + U * np.abs(want)
    err = np.abs(got - want)
    _note(f"time_stretch(factor=1), {'mel' if e2e.mel else 'plain'} helper: largest difference from the float64 analysis + synthesis "
          f"{err.max():.3e}, largest error / bound {(err / bound).max():.3f}; that pair against the input (the DC bin): "
          f"{np.abs(want - x).max():.3e}")
    assert (err <= bound).all()
    assert (np.abs(got - x) <= bound + np.abs(want - x)).all()          # against the input: the DC share, exactly, on top


@pytest.mark.parametrize("factor", [1.5, 2.0])
def test_three_partials_through_the_kernels_agree_with_the_spec(e2e, factor):
    """The experiment of tests/test_stft_stretch_host.py on the device.  The specification runs on the device's own STFT (its
    float32 bits: the peak decisions are properties of those), so the audio may differ by the kernel's bound pushed through
    the synthesis basis plus the synthesis' own error (the Nyquist bin: see below).  The spectral convergence against the ideally stretched sound is
    recorded; the orderings are the host test's."""
    from GANsynth_pytorch.stretch import stretch_positions, time_stretch
    helper, dev = e2e.helper, _dev()
    got = time_stretch(helper, e2e.audio, factor).cpu().numpy().astype(np.float64)
    X, T_all = helper._stft(torch.nn.functional.pad(e2e.audio[None], (0, e2e.extra * HOP)))
    assert T_all == T_E2E + e2e.extra
    pos = torch.cat([stretch_positions(T_E2E, factor=factor), torch.arange(T_E2E, T_all, dtype=torch.float32)])[None].numpy()
    T_out = pos.shape[1] - e2e.extra
    assert got.shape == (T_out * HOP,) and T_out == round(T_E2E * factor)
    spec = S.stretch(X.cpu().numpy(), pos, HOP)
    # the Nyquist bin of a real signal is real: its phase advance is 0 or pi, exactly on the wrap's step, the one place where
    # the float32 and the float64 wrap may take opposite ends.  Its bound is any phase at all, 2 M; every other bin keeps its own.
    assert float(spec.src.margin[..., :-1].min()) >= 1e-5, "a phase advance of this sound sits on the wrap's step"
    bins = spec.bound[0].copy()
    bins[:, -1] = 2 * np.abs(spec.M[0, :, -1])
    want = S.istft(spec.out[0], N_FFT, HOP, T_out * HOP)
    bound = _synthesis_error(e2e, spec.out[0], bins)[:T_out * HOP] + U * np.abs(want)
    err = np.abs(got - want)
    ideal = 0.5 * S.tone(T_out * HOP, 440.0, scale=T_out / T_E2E)
    _note(f"time_stretch(factor={factor}), {'mel' if e2e.mel else 'plain'} helper: largest difference from the float64 spec's audio "
          f"{err.max():.3e}, largest error / bound {(err / bound).max():.3f}; spectral convergence against the ideal "
          f"{S.spectral_convergence(got, ideal, N_FFT, HOP):.4f} (the spec's audio: {S.spectral_convergence(want, ideal, N_FFT, HOP):.4f})")
    assert (err <= bound).all()


@pytest.mark.parametrize("semitones", [3, -4])
def test_transpose_lands_on_the_pitch(e2e, semitones):
    from GANsynth_pytorch.pitch import estimate_pitch
    from GANsynth_pytorch.stretch import transpose, transpose_ratio
    assert transpose(e2e.helper, e2e.audio, 0) is e2e.audio
    y = transpose(e2e.helper, e2e.audio, semitones)
    assert y.shape == e2e.audio.shape and bool(torch.isfinite(y).all())
    midi, confidence = estimate_pitch(y, FS)
    num, den, cents = transpose_ratio(semitones)
    _note(f"transpose({semitones:+d}) = {num}/{den} ({cents:+.3f} cent), {'mel' if e2e.mel else 'plain'} helper: estimated pitch "
          f"{float(midi):.4f} for a target of {69 + semitones}, voiced share {float(confidence):.2f}")
    assert abs(float(midi) - (69 + semitones)) <= 0.05
    both = transpose(e2e.helper, torch.stack([e2e.audio, e2e.audio]), semitones)       # a batch: the same bits per row
    assert torch.equal(both[0], y) and torch.equal(both[1], y)


def test_to_audio_stretched_at_rate_one_is_to_audio(e2e):
    """positions 0 .. T - 1: the decoded STFT is copied bit for bit and the synthesis is `to_audio`'s own call on the same
    rows; asserted within the synthesis bound of both (twice `_synthesis_error`), observed: equal"""
    from GANsynth_pytorch.stretch import stretch_positions
    helper, dev = e2e.helper, _dev()
    spec = helper.to_spectrogram(torch.stack([e2e.audio, e2e.audio.flip(0)]))
    plain = helper.to_audio(spec)
    got = helper.to_audio_stretched(spec, stretch_positions(T_E2E, factor=1).to(dev))
    assert got.shape == plain.shape
    _, (_, a, ph) = helper._to_audio(spec, keep=True)
    from spec_splice_spec import to_stft_f32_model
    Y = to_stft_f32_model(a.cpu().numpy(), ph.cpu().numpy(), int(helper.mel)).astype(np.float64)
    F = N_FFT // 2
    err = np.abs(got.cpu().numpy().astype(np.float64) - plain.cpu().numpy().astype(np.float64))
    for b in range(2):
        bound = 2 * _synthesis_error(e2e, Y[b, :, :F] + 1j * Y[b, :, F:])
        assert (err[b] <= bound).all()
    _note(f"to_audio_stretched at rate 1 against to_audio, {'mel' if e2e.mel else 'plain'} helper: largest difference {err.max():.3e}")
    longer = helper.to_audio_stretched(spec, stretch_positions(T_E2E, factor=1.5).to(dev))
    assert longer.shape == (2, 96 * HOP) and bool(torch.isfinite(longer).all())
    per_item = torch.stack([stretch_positions(T_E2E, n_out=80), stretch_positions(T_E2E, n_out=80, keep_head=8)]).to(dev)
    two = helper.to_audio_stretched(spec, per_item)
    assert torch.equal(two[:1], helper.to_audio_stretched(spec[:1], per_item[0]))
    with pytest.raises(ValueError):
        helper.to_audio_stretched(spec, torch.zeros(3, 80, device=dev))


def test_kept_attack_is_the_source_s_own_frames(e2e):
    """keep_attack_s: the leading frames are copied bit for bit, so the first samples all of whose frames are copied are the
    rate-1 re-synthesis' own up to the synthesis GEMM's summation order"""
    from GANsynth_pytorch.stretch import time_stretch
    same = time_stretch(e2e.helper, e2e.audio, 1.0)
    held = time_stretch(e2e.helper, e2e.audio, 2.0, keep_attack_s=0.04)                 # 10 frames
    assert held.shape == (2 * T_E2E * HOP,)
    n = (10 - e2e.extra) * HOP
    X, _ = e2e.helper._stft(torch.nn.functional.pad(e2e.audio[None], (0, e2e.extra * HOP)))
    Xc = X[0].cpu().numpy().astype(np.float64)
    bound = 2 * _synthesis_error(e2e, Xc[:, :N_FFT // 2] + 1j * Xc[:, N_FFT // 2:])[:n]      # the GEMM runs on other row counts
    diff = (held[:n] - same[:n]).abs().cpu().numpy().astype(np.float64)
    assert (diff <= bound).all() and not torch.equal(held[:20 * HOP], same[:20 * HOP])
    with pytest.raises(ValueError):
        time_stretch(e2e.helper, e2e.audio, 2.0, keep_attack_s=1.0)


# ------------------------------------------------------------- stretch_sound, transpose_sound, the routes: the small model
class _Model:
    """the seeded model of tests/test_code_mix_gpu.py, a helper whose spectrograms are its inputs' size ([2, 64, 128]), and two
    voiced sounds two semitones apart"""

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
        self.audio = torch.from_numpy((0.4 * S.tone(self.n, 880.0)).astype(np.float32))
        self.other = torch.from_numpy((0.4 * S.tone(self.n, 880.0 * 2 ** (2 / 12))).astype(np.float32))


@pytest.fixture(scope="module")
def model():
    return _Model()


def test_transpose_sound(model):
    """`like`: the result must carry the other sound's pitch label, a whole MIDI number, for morphs and searches to compare the
    two at equal pitch: within half a semitone of the other's estimate.  (Observed: a few hundredths.)"""
    import inpainting
    from GANsynth_pytorch.pitch import estimate_pitch
    dev = _dev()
    y, top, bottom = inpainting.transpose_sound(model.m, model.helper, model.audio, like=model.other)
    want_top, want_bottom = inpainting.analyze_audio(model.m, model.helper, model.audio, model.n, dev)
    assert y.shape == (model.n,) and top.shape == want_top.shape and bottom.shape == want_bottom.shape
    target, got, source = (float(estimate_pitch(s.to(dev), 16000)[0]) for s in (model.other, y, model.audio))
    _note(f"transpose_sound(like=): source {source:.3f}, target {target:.3f}, result {got:.3f}")
    assert abs(target - source - 2.0) < 0.1 and abs(got - target) < 0.5
    again = inpainting.analyze_audio(model.m, model.helper, y, model.n, dev)
    assert torch.equal(top, again[0]) and torch.equal(bottom, again[1])
    to_pitch, none_top, none_bottom = inpainting.transpose_sound(model.m, model.helper, model.audio, to_pitch=target, re_encode=False)
    assert torch.equal(to_pitch, y) and none_top is None and none_bottom is None
    by_semitones = inpainting.transpose_sound(model.m, model.helper, model.audio, semitones=-3.5, re_encode=False)[0]
    assert by_semitones.shape == (model.n,)
    noise = 0.1 * torch.randn(model.n, generator=torch.Generator().manual_seed(1))
    for bad in (dict(to_pitch=60.0, audio=noise), dict(like=noise), dict(), dict(semitones=1.0, to_pitch=60.0), dict(to_pitch=float("nan"))):
        with pytest.raises(ValueError):
            inpainting.transpose_sound(model.m, model.helper, **dict(dict(audio=model.audio), **bad))


def test_stretch_sound(model):
    import inpainting
    from GANsynth_pytorch.stretch import time_stretch
    dev = _dev()
    got = inpainting.stretch_sound(model.m, model.helper, audio=model.audio, factor=1.5, keep_attack_s=0.02)
    assert torch.equal(got, time_stretch(model.helper, model.audio.to(dev), 1.5, keep_attack_s=0.02)) and got.shape == (192 * 32,)
    top, bottom = inpainting.analyze_audio(model.m, model.helper, model.audio, model.n, dev)
    same = inpainting.stretch_sound(model.m, model.helper, codes=(top, bottom), factor=1.0)
    plain = inpainting.codes_to_audio(model.m, model.helper, top, bottom)
    assert same.shape == plain.shape and torch.allclose(same, plain, atol=1e-5)
    half = inpainting.stretch_sound(model.m, model.helper, codes=(top, bottom), factor=0.5)
    assert half.shape == (1, model.n // 2) and bool(torch.isfinite(half).all())
    for bad in (dict(), dict(audio=model.audio, codes=(top, bottom)), dict(audio=model.audio, factor=0.0)):
        with pytest.raises(ValueError):
            inpainting.stretch_sound(model.m, model.helper, **dict(dict(factor=2.0), **bad))


def test_routes(model):
    import flask_server
    import inpainting
    app = flask_server.create_app(model.m, None, None, {}, _dev(), spectrograms_helper=model.helper)
    client = app.test_client()
    wav = flask_server._wav_bytes(model.audio, 16000)
    upload, _ = flask_server._read_wav(wav)                               # what the routes see: 16-bit samples
    post = lambda url, **form: client.post(url, data=dict(audio=(io.BytesIO(wav), 'upload.wav'), **form),      # noqa: E731
                                           content_type='multipart/form-data')
    r = post('/transpose-audio?semitones=3')
    assert r.status_code == 200 and r.mimetype == "audio/wav"
    want = inpainting.transpose_sound(model.m, model.helper, upload, semitones=3.0, re_encode=False)[0]
    assert r.data == flask_server._wav_bytes(want, 16000)
    r = post('/transpose-audio', to_pitch='79.5')                         # a form field
    assert r.status_code == 200
    want = inpainting.transpose_sound(model.m, model.helper, upload, to_pitch=79.5, re_encode=False)[0]
    assert r.data == flask_server._wav_bytes(want, 16000)
    noise = flask_server._wav_bytes(0.1 * torch.randn(model.n, generator=torch.Generator().manual_seed(1)), 16000)
    r = client.post('/transpose-audio?to_pitch=60', data=dict(audio=(io.BytesIO(noise), 'noise.wav')), content_type='multipart/form-data')
    assert r.status_code == 400
    r = post('/stretch-audio?factor=1.5&keep_attack_s=0.02')
    assert r.status_code == 200 and r.mimetype == "audio/wav"
    samples, rate = flask_server._read_wav(r.data)
    assert rate == 16000 and samples.numel() == 192 * 32
    want = inpainting.stretch_sound(model.m, model.helper, audio=upload, factor=1.5, keep_attack_s=0.02)
    assert r.data == flask_server._wav_bytes(want, 16000)
    assert post('/stretch-audio?factor=0').status_code == 400
