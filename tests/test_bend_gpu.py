"""Pitch bending on the device (GANsynth_pytorch/bend.py over isi_stft_stretch_f32 and isi_warp_resample_f32,
GANsynth_pytorch.pitch.pitch_contour, inpainting.bend_sound, /bend-audio): the four float64 experiments of
tests/warp_resample_spec.py (tests/test_bend_host.py holds their figures) run through the product on a helper of n_fft 256 /
hop 64 and the same 1 s sounds; the audio is brought to the host, measured with the same tracker and held to the same limits --
at most 1 cent rms and 3 cents max left, the level within 1e-3, the length kept.

Figures of an MI355X run (profiles/bend_checks.txt): flatten 0.332 / 1.109 cents, vibrato 0.244 / 0.856, glide 0.223 / 0.912, the
tracked contour 0.555 / 1.637 (the contour itself 0.441 / 1.059 off the true curve) -- the float64 figures to the digits shown;
`estimate_pitch` hears the flattened sound at 69.0004; `warp` at rate 3/2 differs from `resample` by 5.4e-7, 0.7 % of the two
bounds; a flat tone given the vibrato tone's contour follows it to 0.504 / 1.261 cents.

A recording aid, not a check: with ISI_BEND_RECORD=<file> in the environment the figures are written there when the module ends."""
import io
import os

import numpy as np
import pytest
import torch

import warp_resample_spec as S
from test_bend_host import LEVEL_LIMIT, MAX_LIMIT, RMS_LIMIT

pytestmark = pytest.mark.gpu

NOTES = []
FS, N_FFT, HOP = 16000, 256, 64


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_BEND_RECORD")
    if path and NOTES:
        with open(path, "w") as f:
            f.write("# tests/test_bend_gpu.py on the device: cents left against the ideal pitch (rms / max) and the level ratio,\n"
                    "# beside the float64 figures of tests/test_bend_host.py\n")
            f.writelines(note + "\n" for note in NOTES)


def _note(text):
    print(text)
    NOTES.append(text)


@pytest.fixture(scope="module")
def helper():
    from GANsynth_pytorch.spectrograms_helper import SpectrogramsHelper
    return SpectrogramsHelper(fs_hz=FS, n_fft=N_FFT, hop_length=HOP, window_length=N_FFT).to(_dev())


def _device_bend(helper):
    from GANsynth_pytorch.bend import bend

    def run(x, semis):
        audio = torch.from_numpy((0.5 * x).astype(np.float32)).to(_dev())
        y = bend(helper, audio, torch.from_numpy(np.asarray(semis, dtype=np.float64)).to(_dev()))
        assert y.shape == audio.shape and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
        return 2.0 * y.cpu().numpy().astype(np.float64)
    return run


FLOAT64 = {"flatten": "0.33 / 1.11, level 0.99937", "vibrato": "0.24 / 0.86, level 1.00059", "glide": "0.22 / 0.91, level 1.00039",
           "flatten_tracked": "0.56 / 1.64, level 0.99920"}


def _hold(name, left, level, length):
    _note(f"{name}: left {left[0]:.3f} / {left[1]:.3f} cents, level ratio {level:.5f}   (float64: {FLOAT64[name]})")
    assert left[0] <= RMS_LIMIT and left[1] <= MAX_LIMIT
    assert abs(level - 1.0) <= LEVEL_LIMIT
    assert length == S.N_EXP


@pytest.mark.parametrize("name", ["flatten", "vibrato", "glide"])
def test_known_curves_on_the_device(helper, name):
    r = getattr(S, "experiment_" + name)(bend_fn=_device_bend(helper))
    _hold(name, r.left, r.level, r.length)


def test_flatten_by_the_tracked_contour_on_the_device(helper):
    """the 30-cents-sharp vibrato tone through `bend_sound(flatten=True, to_pitch=69)`: `pitch_contour`, `contour_curve`, `bend`;
    then `estimate_pitch` hears MIDI 69 within 0.05 semitone"""
    import inpainting
    from GANsynth_pytorch.pitch import estimate_pitch, pitch_contour
    dev = _dev()
    own = 0.30 + S.vibrato_curve(S.N_EXP)
    x = S.tone_along(own)
    audio = torch.from_numpy((0.5 * x).astype(np.float32)).to(dev)
    clip = float(estimate_pitch(audio, FS)[0])
    track = pitch_contour(audio, FS)
    W = 448
    assert track.midi.shape == track.voiced.shape == (1, (3 * S.N_EXP - W - 158) // (W // 4) + 1) and abs(clip - 69.3) < 0.1
    seen = inpainting.contour_curve(track, clip, S.N_EXP, FS).numpy()
    off = 100.0 * (seen - 69.0 - own)[S.TRIM:-S.TRIM]
    y, top, bottom = inpainting.bend_sound(None, helper, audio, flatten=True, to_pitch=69.0, re_encode=False)
    assert top is None and bottom is None and y.shape == audio.shape
    got = 2.0 * y.cpu().numpy().astype(np.float64)
    _note(f"pitch_contour (W = {W}): off the true curve by {np.sqrt(np.mean(off ** 2)):.3f} / {np.abs(off).max():.3f} cents   (float64: 0.44 / 1.06)")
    _hold("flatten_tracked", S.track_cents(got, 0.0), S.level_ratio(got, x), len(got))
    midi, confidence = estimate_pitch(y, FS)
    _note(f"bend_sound(flatten, to_pitch=69): estimate_pitch hears {float(midi):.4f} (the source: {clip:.4f}), voiced share {float(confidence):.2f}")
    assert abs(float(midi) - 69.0) <= 0.05
    # without to_pitch the target is the clip's own rounded pitch: the same here
    again = inpainting.bend_sound(None, helper, audio, flatten=True, re_encode=False)[0]
    assert torch.equal(again, y)
    # another sound's contour: a flat tone takes the vibrato of this one
    flat = torch.from_numpy((0.5 * S.tone_along(np.zeros(S.N_EXP))).astype(np.float32)).to(dev)
    sung = inpainting.bend_sound(None, helper, flat, contour_of=audio, re_encode=False)[0]
    left = S.track_cents(2.0 * sung.cpu().numpy().astype(np.float64), own - np.median(own))
    _note(f"bend_sound(contour_of=): left {left[0]:.3f} / {left[1]:.3f} cents against the other sound's own deviation")
    assert left[0] <= 2 * RMS_LIMIT and left[1] <= 2 * MAX_LIMIT      # the contour's error and the bend's, one each
    noise = 0.1 * torch.randn(S.N_EXP, generator=torch.Generator().manual_seed(1)).to(dev)
    for bad in (dict(flatten=True), dict(contour_of=noise)):
        with pytest.raises(ValueError):
            inpainting.bend_sound(None, helper, **dict(dict(audio=noise if "flatten" in bad else flat, re_encode=False), **bad))
    with pytest.raises(ValueError):
        pitch_contour(noise, FS)


def test_warp_at_a_constant_rate_is_resample(helper):
    """`warp` along n 3/2 under the default cutoff against `resample(x, 3, 2)`: within the sum of the two kernels' bounds"""
    import resample_spec as RS
    from GANsynth_pytorch.bend import default_cutoff, warp
    from GANsynth_pytorch.resample import resample
    dev = _dev()
    g = np.random.default_rng(3)
    x = g.standard_normal((2, 1000)).astype(np.float32)
    pos, cut = S.constant_rate_rows(1000, 3, 2)
    xd, pd = torch.from_numpy(x).to(dev), torch.from_numpy(pos).to(dev)
    got = warp(xd, pd)
    assert got.shape == (2, len(pos)) and got.dtype == torch.float32
    used = default_cutoff(pd[None]).cpu().numpy()
    assert np.abs(used - cut).max() <= 2.0 ** -24                      # the central differences of n 3/2 are 3/2
    spec = S.warp(x, pos[None], used)
    S.compare(got.cpu().numpy(), spec, "warp at 3/2")
    _, scale = RS.resample(x, 3, 2, with_abs=True)
    taps = RS.geometry(3, 2)[3]
    both = spec.bound + ((taps + 2) * 2.0 ** -24 + 2.0 ** -23) * scale        # + an ulp on every coefficient of the product's table
    err = np.abs(got.cpu().numpy().astype(np.float64) - resample(xd, 3, 2).cpu().numpy().astype(np.float64))
    _note(f"warp at rate 3/2 against resample: largest difference {err.max():.3e}, {(err / both).max():.3f} of the two bounds")
    assert (err <= both).all()
    # one row, per-row maps, an explicit cutoff
    assert torch.equal(warp(xd[0], pd), got[0]) and torch.equal(warp(xd, torch.stack([pd, pd])), got)
    assert torch.equal(warp(xd, pd, torch.from_numpy(used[0]).to(dev)), got)
    with pytest.raises(ValueError):
        warp(xd, torch.zeros(3, 5, dtype=torch.float64, device=dev))


def test_zero_curve_returns_the_input_and_batches_agree(helper):
    from GANsynth_pytorch.bend import bend, glide, vibrato
    dev = _dev()
    x = torch.from_numpy((0.5 * S.tone_along(np.zeros(4000))).astype(np.float32)).to(dev)
    assert bend(helper, x, 0.0) is x and bend(helper, x, torch.zeros(4000, dtype=torch.float64, device=dev)) is x
    assert vibrato(helper, x, 6.0, 0.0) is x and glide(helper, x, 0.0, 0.0) is x
    y = glide(helper, x, -1.0, 2.0, start_s=0.05, end_s=0.2)
    both = glide(helper, torch.stack([x, x]), -1.0, 2.0, start_s=0.05, end_s=0.2)
    assert y.shape == x.shape and both.shape == (2, 4000) and torch.equal(both[0], y) and torch.equal(both[1], y)
    v = vibrato(helper, x[:1001], 5.0, 30.0, onset_s=0.01, ramp_s=0.02)            # a length that is no multiple of the hop
    assert v.shape == (1001,) and bool(torch.isfinite(v).all())


def test_route():
    """/bend-audio on the seeded small model of tests/test_stft_stretch_gpu.py: a WAV of the input's length, the bytes of
    `bend_sound`'s result"""
    import flask_server
    import inpainting
    from test_stft_stretch_gpu import _Model
    model = _Model()
    client = flask_server.create_app(model.m, None, None, {}, _dev(), spectrograms_helper=model.helper).test_client()
    wav = flask_server._wav_bytes(model.audio, 16000)
    upload, _ = flask_server._read_wav(wav)
    post = lambda url, **form: client.post(url, data=dict(audio=(io.BytesIO(wav), 'upload.wav'), **form),      # noqa: E731
                                           content_type='multipart/form-data')
    for url, form, kw in (("/bend-audio?vibrato_hz=5.5&vibrato_cents=40", {}, dict(vibrato=(5.5, 40.0))),
                          ("/bend-audio", dict(glide_from="-1", glide_to="2.5"), dict(glide=(-1.0, 2.5))),
                          ("/bend-audio?flatten=1&to_pitch=82", {}, dict(flatten=True, to_pitch=82.0)),
                          ("/bend-audio?flatten=1", {}, dict(flatten=True))):
        r = post(url, **form)
        assert r.status_code == 200 and r.mimetype == "audio/wav", url
        samples, rate = flask_server._read_wav(r.data)
        assert rate == 16000 and samples.numel() == model.n
        want = inpainting.bend_sound(model.m, model.helper, upload, re_encode=False, **kw)[0]
        assert r.data == flask_server._wav_bytes(want, 16000)
    y, top, bottom = inpainting.bend_sound(model.m, model.helper, upload, vibrato=(5.5, 40.0))
    want_top, want_bottom = inpainting.analyze_audio(model.m, model.helper, y, model.n, _dev())
    assert torch.equal(top, want_top) and torch.equal(bottom, want_bottom)
    noise = flask_server._wav_bytes(0.1 * torch.randn(model.n, generator=torch.Generator().manual_seed(1)), 16000)
    r = client.post('/bend-audio?flatten=1', data=dict(audio=(io.BytesIO(noise), 'noise.wav')), content_type='multipart/form-data')
    assert r.status_code == 400
