"""The pitch kernels (csrc/pitch.hip: isi_pitch_difference_f32, isi_pitch_pick_f32) against the float64 specification of
tests/pitch_spec.py, and the surfaces built on them (`GANsynth_pytorch.pitch.estimate_pitch`, `inpainting.estimate_pitch`,
the /analyze-audio route without a `pitch` argument).  The comparisons and their bounds are derived in
tests/pitch_checks.py, and tests/test_pitch_host.py shows that each rejects a planted fault:
  impulses    every d is exactly 0, 1 or 2 and every energy 0 or 1: pins every index and both frame edges bit-exactly;
  noise       |d - d64| <= (W + 4) 2^-24 d64 per entry, W fp32 fma steps on rounded non-negative terms, in any order;
  pick        on frames whose every comparison has a relative gap above 4 (tau_max + 2) 2^-24 -- at least 95 % of them
              -- the aperiodicity within that factor of d'64(tau*) and the period within the first-order bound of the
              fp32 vertex formula, u' (|o| (3 + |a - 2 b| / v) + |tau* + o|): the lag itself is the float64 one.
Measured on an MI355X (profiles/pitch_checks.txt): difference errors at most 0.12 of the bound (0.016 at the default
constants); 0.026 of the pick frames uncertified, aperiodicity at most 0.017 of its bound, period at most 0.988 of its
bound (the bound ends in the rounding of tau* + o to fp32 and is reached where that rounding is at its worst); MIDI 21,
60.3 and 108 estimated as 21.0000, 60.3005 and 108.0023, the spec's own figures."""
import io

import numpy as np
import pytest
import torch

import pitch_checks as K
import pitch_spec as S
from test_prior_gpu import _dev
from test_resample_gpu import _app, _view

pytestmark = pytest.mark.gpu

SMALL = [(64, 16, 40), (64, 16, 41), (67, 5, 1030)]      # (W, hop, tau_max); the last: W % 4 != 0, two workgroups per frame


def _lengths(w, hop, tau_max):
    """The last frame ends exactly at L (4 frames); one sample short of a fifth frame; a single frame."""
    return [w + tau_max + 3 * hop, w + tau_max + 4 * hop - 1, w + tau_max]


def _difference(x, w, hop, tau_max):
    from GANsynth_pytorch import pitch as PT
    d, e = PT.difference(x, w, hop, tau_max)
    torch.cuda.synchronize()
    return d, e


@pytest.mark.parametrize("w,hop,tau_max", SMALL)
def test_impulses_are_bit_exact(w, hop, tau_max):
    dev = _dev()
    for L in _lengths(w, hop, tau_max):
        positions = [0, L - 1, w - 1, w, hop + w - 1, tau_max, L // 2]
        wide = torch.zeros(len(positions), L + 7)
        for b, p in enumerate(positions):
            wide[b, 3 + p] = 1.0
        x = wide.to(dev)[:, 3:3 + L]
        assert not x.is_contiguous()
        d, e = _difference(x, w, hop, tau_max)
        assert d.shape == (len(positions), S.frames(L, w, hop, tau_max), tau_max + 1)
        for b in range(len(positions)):
            K.compare_difference(d[b].cpu().numpy(), e[b].cpu().numpy(), x[b].cpu().numpy(), w, hop, tau_max, exact=True)


@pytest.mark.parametrize("w,hop,tau_max", SMALL)
def test_noise_against_the_float64_spec_and_batch_invariance(w, hop, tau_max):
    dev = _dev()
    for L in _lengths(w, hop, tau_max):
        x = _view(3, L, dev, seed=L + tau_max)             # row stride L + 7, first sample 3 floats into the wider tensor
        d, e = _difference(x, w, hop, tau_max)
        share = max(K.compare_difference(d[b].cpu().numpy(), e[b].cpu().numpy(), x[b].cpu().numpy(), w, hop, tau_max)
                    for b in range(3))
        print(f"CHECK difference W={w} hop={hop} tau_max={tau_max} L={L} B=3: largest err / bound {share:.3f}")
        for b in range(3):                                 # a row of the batch is bit-equal to the same row alone
            d1, e1 = _difference(x[b:b + 1], w, hop, tau_max)
            assert torch.equal(d1[0], d[b]) and torch.equal(e1[0], e[b])
        dc, ec = _difference(x.contiguous(), w, hop, tau_max)
        assert torch.equal(dc, d) and torch.equal(ec, e)


def test_difference_at_the_default_constants():
    dev = _dev()
    x = _view(2, 12000, dev, seed=5)
    d, e = _difference(x, S.W, S.HOP, S.TAU_MAX)
    assert d.shape == (2, 10, S.TAU_MAX + 1) and e.shape == (2, 10)
    share = max(K.compare_difference(d[b].cpu().numpy(), e[b].cpu().numpy(), x[b].cpu().numpy(), S.W, S.HOP, S.TAU_MAX)
                for b in range(2))
    print(f"CHECK difference W={S.W} hop={S.HOP} tau_max={S.TAU_MAX} L=12000 B=2: largest err / bound {share:.3f}")
    d1, e1 = _difference(x[1:2], S.W, S.HOP, S.TAU_MAX)
    assert torch.equal(d1[0], d[1]) and torch.equal(e1[0], e[1])


def test_pick_against_the_float64_choice():
    from GANsynth_pytorch import pitch as PT
    dev = _dev()
    d32, kinds = K.pick_frames()
    period, ap = PT.pick(torch.from_numpy(d32).to(dev), S.TAU_MIN, S.THR)
    torch.cuda.synchronize()
    period, ap = period.cpu().numpy(), ap.cpu().numpy()
    uncertified, p_share, ap_share = K.compare_pick(period, ap, d32, S.TAU_MIN, S.TAU_MAX, S.THR)
    print(f"CHECK pick tau_min={S.TAU_MIN} tau_max={S.TAU_MAX} thr={S.THR} frames={len(kinds)}: uncertified share "
          f"{uncertified:.3f}, largest period err / bound {p_share:.3f}, largest aperiodicity err / bound {ap_share:.3f}")
    # silence: d = 0 gives cs = 0 and d' = 1 exactly, in any arithmetic: the first lag, untouched by the vertex
    assert (period[kinds == "silence"] == S.TAU_MIN).all() and (ap[kinds == "silence"] == 1).all()
    # a frame alone and a batch of frames agree bit for bit
    one, one_ap = PT.pick(torch.from_numpy(d32[37:38]).to(dev), S.TAU_MIN, S.THR)
    assert one.item() == period[37] and one_ap.item() == ap[37]


def test_pick_on_a_short_row_of_lags():
    """n = tau_max + 1 = 42 lags, fewer than the workgroup's threads: periodic noise of period 9 .. 20 samples."""
    from GANsynth_pytorch import pitch as PT
    dev = _dev()
    w, hop, tau_max, tau_min, thr = 64, 16, 41, 2, 0.1
    rng = np.random.default_rng(11)
    rows = []
    for period_n in range(9, 21):
        cell = rng.standard_normal(period_n)
        x = np.tile(cell, 40)[:w + tau_max + 7 * hop] + 0.01 * rng.standard_normal(w + tau_max + 7 * hop)
        rows.append(S.difference(x.astype(np.float32).astype(np.float64), w, hop, tau_max)[0])
    rows.append(S.difference(rng.standard_normal(w + tau_max + 7 * hop), w, hop, tau_max)[0])     # the fallback
    d32 = np.concatenate(rows).astype(np.float32)
    period, ap = PT.pick(torch.from_numpy(d32).to(dev), tau_min, thr)
    torch.cuda.synchronize()
    uncertified, p_share, ap_share = K.compare_pick(period.cpu().numpy(), ap.cpu().numpy(), d32, tau_min, tau_max, thr)
    print(f"CHECK pick tau_min={tau_min} tau_max={tau_max} thr={thr} frames={d32.shape[0]}: uncertified share "
          f"{uncertified:.3f}, largest period err / bound {p_share:.3f}, largest aperiodicity err / bound {ap_share:.3f}")


def test_estimate_pitch_end_to_end():
    from GANsynth_pytorch import pitch as PT
    dev = _dev()
    truth = [21, 60.3, 108]
    tones = [K.tone(m, "harmonic", seed=i).astype(np.float32) for i, m in enumerate(truth)]
    want = [S.estimate(t.astype(np.float64), 16000) for t in tones]
    wide = torch.zeros(3, 8000 + 7)
    for b, t in enumerate(tones):
        wide[b, 3:8003] = torch.from_numpy(t)
    batch = wide.to(dev)[:, 3:8003]
    assert not batch.is_contiguous()
    midi_b, conf_b, track = PT.estimate_pitch(batch, 16000, return_track=True)
    assert midi_b.shape == conf_b.shape == (3,) and midi_b.dtype == torch.float32
    T = S.frames(24000)
    assert track.midi.shape == track.aperiodicity.shape == track.energy.shape == track.voiced.shape == (3, T)
    assert torch.allclose(track.times_s.cpu(), (torch.arange(T) * S.HOP + S.W / 2) / S.FS_A)
    for b, (t, m) in enumerate(zip(tones, truth)):
        midi, conf = PT.estimate_pitch(torch.from_numpy(t).to(dev), 16000)
        assert midi.shape == () and abs(midi.item() - m) < 0.05 and abs(midi.item() - want[b][0]) < 0.01
        assert conf.item() == want[b][1] == 1.0
        assert abs(midi_b[b].item() - m) < 0.05 and abs(midi_b[b].item() - want[b][0]) < 0.01 and conf_b[b].item() == 1.0
        print(f"CHECK estimate_pitch MIDI {m}: {midi.item():.4f} (spec {want[b][0]:.4f})")
    g = torch.Generator().manual_seed(2)
    noise = (torch.randn(2, 8000, generator=g) * 0.3).to(dev)
    noise[1] = 0.0                                          # and silence
    midi, conf = PT.estimate_pitch(noise, 16000)
    assert torch.isnan(midi).all() and (conf == 0).all()
    short, short_conf = PT.estimate_pitch(torch.zeros(10, device=dev), 48000)      # padded to one frame; no resampling
    assert torch.isnan(short) and short_conf.item() == 0
    with pytest.raises(ValueError, match="16000|48000"):
        PT.estimate_pitch(torch.zeros(2000, device=dev), 44101)                    # the resampler's refusal passes through


def test_inpainting_estimate_pitch_and_the_analyze_audio_route(golden_dir):
    import flask_server
    import inpainting
    c, vq, top, bottom, helper, dev = _app(golden_dir)
    tone = torch.from_numpy(K.tone(69, "harmonic", seconds=0.5).astype(np.float32))
    assert inpainting.estimate_pitch(tone.to(dev), helper) == (69, 1.0)
    assert inpainting.estimate_pitch(tone.to(dev), helper, fs_hz=16000, pitch_range=range(24, 61)) == (60, 1.0)
    assert inpainting.estimate_pitch(tone.to(dev), helper, pitch_range=[72, 80, 75])[0] == 72
    g = torch.Generator().manual_seed(4)
    noise = torch.randn(8000, generator=g) * 0.3
    assert inpainting.estimate_pitch(noise.to(dev), helper) == (None, 0.0)

    def post(wav, query):
        return c.post("/analyze-audio" + query, data={"audio": (io.BytesIO(wav), "note.wav")},
                      content_type="multipart/form-data")
    wav = flask_server._wav_bytes(tone, 16000)
    # with a pitch: what the route answered before it could estimate one
    given = post(wav, "?pitch=60&instrument_family_str=fam2")
    assert given.status_code == 200
    x, rate = flask_server._read_wav(wav)
    res_n = inpainting.top_resolution_n(vq, top, bottom, helper, dev)
    dur = inpainting.adapt_duration(x.numel(), 16000, 4.0, res_n, top.shape[1])
    t, b = inpainting.analyze_audio(vq, helper, x, dur, dev)
    values = {"pitch": 60, "instrument_family_str": "fam2"}
    assert given.get_json() == {
        "top_code": t[0].int().cpu().numpy().tolist(), "bottom_code": b[0].int().cpu().numpy().tolist(),
        "top_conditioning": {k: [[v] * top.shape[1]] * top.shape[0] for k, v in values.items()},
        "bottom_conditioning": {k: [[v] * bottom.shape[1]] * bottom.shape[0] for k, v in values.items()}}
    # without one, and with pitch=auto: the estimate fills the maps; the codes do not change
    for query in ("?instrument_family_str=fam2", "?pitch=auto&instrument_family_str=fam2"):
        r = post(wav, query)
        assert r.status_code == 200
        body = r.get_json()
        assert body["top_conditioning"]["pitch"] == [[69] * top.shape[1]] * top.shape[0]
        assert body["bottom_conditioning"]["pitch"] == [[69] * bottom.shape[1]] * bottom.shape[0]
        assert body["top_code"] == given.get_json()["top_code"] and body["bottom_code"] == given.get_json()["bottom_code"]
        assert body["top_conditioning"]["instrument_family_str"] == given.get_json()["top_conditioning"]["instrument_family_str"]
    # a 48 kHz upload of the same note: estimated from the converted samples
    from GANsynth_pytorch.resample import resample
    up = resample(tone.to(dev), 16000, 48000).cpu()
    r = post(flask_server._wav_bytes(up, 48000), "?instrument_family_str=fam2")
    assert r.status_code == 200 and r.get_json()["top_conditioning"]["pitch"][0][0] == 69
    # noise has no pitch: 400, and the message says which argument to give
    bad = post(flask_server._wav_bytes(noise, 16000), "?instrument_family_str=fam2")
    assert bad.status_code == 400 and b"pitch" in bad.data
    assert post(flask_server._wav_bytes(noise, 16000), "?pitch=64&instrument_family_str=fam2").status_code == 200
