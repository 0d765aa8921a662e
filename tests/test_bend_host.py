"""Host-side checks of pitch bending (GANsynth_pytorch/bend.py, inpainting.bend_sound, /bend-audio): the float64 arithmetic of
tests/warp_resample_spec.py -- the stretch specification's STFT, phase-locked re-timing and inverse, then the time-warped read
-- flattens a vibrato, adds one, glides and flattens by a tracked contour to within a cent; three planted faults of the path do
not; `bend_maps` is that arithmetic's maps; bad arguments are refused before any launch.  No GPU needed.

Float64 figures, cents (rms / max) left against the ideal pitch, 1 s at 16 kHz, 1500 samples dropped at each end:
    +-50 cent 6 Hz vibrato flattened with its known curve   0.33 / 1.11   (source 35.7 / 50.5; level ratio 0.99937)
    the same vibrato added to a flat tone                   0.24 / 0.86   (level 1.00059)
    a linear glide of +3 semitones                          0.22 / 0.91   (level 1.00039)
    30 cents sharp + vibrato, flattened by its YIN contour  0.56 / 1.64   (W = 448; the contour itself is off by 0.44 / 1.06)
    the same with 64 ms windows (W = 3008)                  8.50 / 13.06  (the contour: 8.57 / 12.92)"""
import functools
import io
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import warp_resample_spec as S

RMS_LIMIT, MAX_LIMIT, LEVEL_LIMIT = 1.0, 3.0, 1e-3


@functools.lru_cache(maxsize=None)
def _experiment(name, **kw):
    return getattr(S, "experiment_" + name)(**kw)


@pytest.mark.parametrize("name", ["flatten", "vibrato", "glide", "flatten_tracked"])
def test_float64_experiments_stay_within_a_cent(name):
    r = _experiment(name)
    print(f"{name}: left {r.left[0]:.3f} / {r.left[1]:.3f} cents (rms / max), untreated {r.source[0]:.1f} / {r.source[1]:.1f}, "
          f"level ratio {r.level:.5f}" + (f", contour error {r.contour_error[0]:.2f} / {r.contour_error[1]:.2f}" if name == "flatten_tracked" else ""))
    assert r.left[0] <= RMS_LIMIT and r.left[1] <= MAX_LIMIT
    assert abs(r.level - 1.0) <= LEVEL_LIMIT
    assert r.length == S.N_EXP
    assert r.source[0] > 30.0                     # the untreated sound is tens of cents away: the experiment has something to do


def test_the_contour_needs_its_own_window():
    """with the clip estimator's 64 ms window the contour averages the vibrato away and the flattened sound keeps most of it"""
    r = _experiment("flatten_tracked", w=3008)
    print(f"64 ms windows: left {r.left[0]:.2f} / {r.left[1]:.2f} cents, contour error {r.contour_error[0]:.2f} / {r.contour_error[1]:.2f}")
    assert r.left[0] > RMS_LIMIT
    assert r.contour_error[0] > 5.0 * _experiment("flatten_tracked").contour_error[0]


@pytest.mark.parametrize("mutant", ["no_stretch", "warp_sign", "positions_from_phi"])
def test_planted_faults_miss_the_limits(mutant):
    """on the 30-cents-sharp vibrato tone flattened with its known curve: the path as specified meets the limits, without the
    compensating stretch / with the curve's sign flipped in the warp only / with frame positions from phi instead of phi^-1 it
    does not"""
    good = _experiment("flatten", sharp_cents=30.0)
    assert good.left[0] <= RMS_LIMIT and good.left[1] <= MAX_LIMIT and abs(good.level - 1.0) <= LEVEL_LIMIT
    bad = _experiment("flatten", sharp_cents=30.0, mutant=mutant)
    print(f"{mutant}: left {bad.left[0]:.2f} / {bad.left[1]:.2f} cents (as specified: {good.left[0]:.2f} / {good.left[1]:.2f})")
    assert bad.left[0] > RMS_LIMIT or bad.left[1] > MAX_LIMIT


def test_bend_maps_against_float64_numpy():
    from GANsynth_pytorch import bend as B
    L, fs, hop = 5000, 16000, 64
    # control points: linear between, held outside
    times, values = [0.05, 0.1, 0.25], [0.0, 2.0, -1.5]
    at = np.arange(L) / fs
    want_curve = np.interp(at, times, values)
    got_curve = B.curve(L, values, times, fs).numpy()
    assert got_curve.dtype == np.float64 and np.abs(got_curve - want_curve).max() <= 1e-12
    assert got_curve[0] == 0.0 and got_curve[-1] == -1.5
    r, phi, frames = B.bend_maps(L, values, times, fs, hop)
    wr, wphi, wframes = S.curve_maps(want_curve, hop)
    assert r.dtype == phi.dtype == frames.dtype == torch.float64
    assert np.abs(r.numpy() - wr).max() <= 1e-12 and np.abs(phi.numpy() - wphi).max() <= 1e-8
    assert frames.shape == wframes.shape and np.abs(frames.numpy() - wframes).max() <= 1e-9
    assert phi[0] == 0.0 and frames[0] == 0.0 and frames.numel() == math.ceil(float(wphi[-1] + wr[-1]) / hop)
    # phi^-1: phi interpolated at the frames' source positions gives j hop back
    src = frames.numpy() * hop
    i = np.minimum(np.floor(src).astype(int), L - 1)
    assert np.abs(wphi[i] + (src - i) * wr[i] - np.arange(len(src)) * hop).max() <= 1e-7
    # per-sample and constant curves; the vibrato and glide curves
    per_sample = S.vibrato_curve(L)
    assert np.abs(B.curve(L, per_sample).numpy() - per_sample).max() == 0.0
    assert torch.equal(B.curve(7, 1.5), torch.full((7,), 1.5, dtype=torch.float64))
    v = B.vibrato_curve(L, fs, 6.0, 50.0, onset_s=0.1, ramp_s=0.05).numpy()
    t = at - 0.1
    assert np.abs(v - 0.5 * np.clip(t / 0.05, 0.0, 1.0) * np.sin(2 * np.pi * 6.0 * t)).max() <= 1e-12 and not v[:1600].any()
    r1 = B.bend_maps(L, 12.0, None, fs, hop)[0]
    assert torch.equal(r1, torch.full((L,), 2.0, dtype=torch.float64))
    pos = torch.tensor([[0.0, 1.0, 2.5, 5.5, 8.5]], dtype=torch.float64)
    cut = B.default_cutoff(pos)
    assert cut.dtype == torch.float32
    assert np.allclose(cut.numpy(), S.ROLLOFF / np.array([[1.0, 1.25, 2.25, 3.0, 3.0]]), rtol=1e-7)


def test_argument_refusals():
    from GANsynth_pytorch import bend as B
    from interactive_spectrogram_inpainting import _hip
    helper = SimpleNamespace(fs_hz=16000, n_fft=256, hop_length=64)
    x = torch.zeros(1000)
    for bad in (float("nan"), float("inf"), 24.5, -30.0):
        with pytest.raises(ValueError):
            B.curve(10, bad)
        with pytest.raises(ValueError):
            B.bend(helper, x, [0.0, bad], [0.0, 0.05])
    with pytest.raises(ValueError):
        B.curve(10, [1.0, 2.0, 3.0])                                  # neither 1 nor L values
    with pytest.raises(ValueError):
        B.curve(10, [1.0, 2.0], [0.0])                                # values and times differ in number
    with pytest.raises(ValueError):
        B.curve(10, [1.0, 2.0], [0.5, 0.5])                           # times not ascending
    with pytest.raises(ValueError):
        B.curve(0, 1.0)
    with pytest.raises(ValueError):
        B.bend_maps(10, 1.0, None, 16000, 0)
    with pytest.raises(ValueError):
        B.bend(helper, torch.zeros(2, 3, 4), 1.0)
    with pytest.raises(ValueError):
        B.glide(helper, x, 0.0, 1.0, start_s=0.5, end_s=0.5)
    with pytest.raises(ValueError):
        B.vibrato(helper, x, -1.0, 50.0)
    with pytest.raises(ValueError):
        B.vibrato(helper, x, 6.0, float("nan"))
    # the zero curve returns the input itself, wherever it lives; anything else has no CPU path
    assert B.bend(helper, x, 0.0) is x and B.bend(helper, x, [0.0, 0.0], [0.0, 0.01]) is x and B.vibrato(helper, x, 6.0, 0.0) is x
    with pytest.raises(_hip.HipLibraryError):
        B.bend(helper, x, 1.0)
    with pytest.raises(_hip.HipLibraryError):
        B.warp(x, torch.arange(10, dtype=torch.float64))


def test_contour_curve_fills_rejected_frames_from_their_neighbours():
    import inpainting
    from GANsynth_pytorch.pitch import PitchTrack
    midi = torch.tensor([[69.2, 69.4, 81.3, 69.0, 40.0, 68.8]])         # an octave error, and an unvoiced frame
    voiced = torch.tensor([[True, True, True, True, False, True]])
    times = torch.arange(6, dtype=torch.float32) * 0.01 + 0.005
    track = PitchTrack(midi, torch.zeros_like(midi), torch.ones_like(midi), voiced, times)
    got = inpainting.contour_curve(track, 69.1, 1120, 16000).numpy()
    want = np.interp(np.arange(1120) / 16000.0, times.double().numpy(), np.array([69.2, 69.4, 69.4, 69.0, 69.0, 68.8], dtype=np.float32).astype(np.float64))
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12
    assert got[0] == np.float32(69.2) and got[-1] == np.float32(68.8)  # held outside the frame times
    with pytest.raises(ValueError):
        inpainting.contour_curve(track, 75.0, 100, 16000, max_correction=1.0)
    x = torch.zeros(100)
    for bad in (dict(), dict(vibrato=(6.0, 50.0), flatten=True), dict(glide=(0.0, 1.0), to_pitch=69.0), dict(curve=[0.0], times_s=[0.0], glide=(0.0, 1.0))):
        with pytest.raises(ValueError):
            inpainting.bend_sound(None, SimpleNamespace(fs_hz=16000, device=None), x, **bad)


def test_route_refuses_bad_arguments():
    import flask_server
    helper = SimpleNamespace(fs_hz=16000, n_fft=128, hop_length=32, device=None)
    client = flask_server.create_app(None, None, None, {}, "cpu", spectrograms_helper=helper).test_client()
    wav = flask_server._wav_bytes(torch.zeros(400), 16000)
    post = lambda url: client.post(url, data=dict(audio=(io.BytesIO(wav), 'upload.wav')), content_type='multipart/form-data')   # noqa: E731
    for url in ("/bend-audio", "/bend-audio?vibrato_hz=6", "/bend-audio?vibrato_cents=50", "/bend-audio?glide_from=1",
                "/bend-audio?vibrato_hz=6&vibrato_cents=50&flatten=1", "/bend-audio?glide_from=0&glide_to=1&vibrato_hz=6&vibrato_cents=5",
                "/bend-audio?vibrato_hz=six&vibrato_cents=50", "/bend-audio?glide_from=0&glide_to=1&to_pitch=69", "/bend-audio?flatten=0",
                "/bend-audio?to_pitch=69", "/bend-audio?glide_from=0&glide_to=30", "/bend-audio?vibrato_hz=-6&vibrato_cents=50"):
        assert post(url).status_code == 400, url
    assert client.post("/bend-audio?flatten=1").status_code == 400                    # no upload
    assert client.post("/bend-audio?glide_from=0&glide_to=1", data=dict(audio=(io.BytesIO(b"nonsense"), 'x.wav')),
                       content_type='multipart/form-data').status_code == 400
    without = flask_server.create_app(None, None, None, {}, "cpu").test_client()
    assert without.post("/bend-audio?flatten=1").status_code == 501
