"""Host-side checks of the pitch estimator (GANsynth_pytorch/pitch.py, csrc/pitch.hip): the written specification
(tests/pitch_spec.py) finds the pitch of synthetic tones and calls noise and silence unvoiced, the comparisons of
tests/test_pitch_gpu.py (tests/pitch_checks.py) accept a faithful fp32 evaluation and reject planted faults, and the
library refuses bad arguments before any launch.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import pitch_checks as K
import pitch_spec as S

FAKE = 0x10000      # non-null, 16-byte aligned, never dereferenced on the host
PITCHES = (21, 28.5, 36, 45.3, 54, 60.3, 66, 72.7, 84, 96, 102, 108)


@pytest.mark.parametrize("timbre", K.TIMBRES)
def test_spec_finds_the_pitch_of_synthetic_tones(timbre):
    """0.5 s tones at 16 kHz (pitch_checks.tone), twelve pitches from MIDI 21 to 108, four of them detuned, white noise at
    0.003 and 0.02 of full scale: |pitch - truth| < 0.05 semitone and every frame voiced.  Measured with this spec over the
    72 tones: worst error 0.0104 semitone.  The 16 kHz estimator with integer lags this replaces
    made octave errors from MIDI 54 up."""
    worst = 0.0
    for midi in PITCHES:
        for noise in (0.003, 0.02):
            pitch, confidence = S.estimate(K.tone(midi, timbre, noise=noise), 16000)
            worst = max(worst, abs(pitch - midi))
            assert abs(pitch - midi) < 0.05, (timbre, midi, noise, pitch)
            assert confidence == 1.0
    print(f"{timbre}: worst error {worst:.4f} semitone")


def test_spec_noise_and_silence_are_unvoiced_and_a_weak_fundamental_is_no_octave_error():
    rng = np.random.default_rng(1)
    for x in (0.3 * rng.standard_normal(8000), np.zeros(8000), np.zeros(100)):
        pitch, confidence = S.estimate(x, 16000)
        assert pitch != pitch and confidence == 0.0
    # an octave up would be + 12: MIDI 102 with the fundamental 16 dB down has partials at f0 and 2 f0 only
    for midi in (60, 90, 102):
        pitch, _ = S.estimate(K.tone(midi, "weak_fundamental"), 16000)
        assert abs(pitch - midi) < 0.05
    # the definition and the quick route are one function
    x = S.analysis_signal(K.tone(60.3, "harmonic", seconds=0.2), 16000)[:S.W + S.TAU_MAX + 2 * S.HOP]
    (d1, e1), (d2, e2) = S.difference(x), S.difference_by_correlation(x)
    assert d1.shape == (3, S.TAU_MAX + 1) and np.abs(d1 - d2).max() <= 1e-12 * e1.max() and np.allclose(e1, e2, rtol=1e-14)
    assert S.estimate(K.tone(60.3, "harmonic", seconds=0.2), 16000, direct=True)[0] == pytest.approx(
        S.estimate(K.tone(60.3, "harmonic", seconds=0.2), 16000)[0], abs=1e-9)
    # lower median and the voiced share
    pitch, confidence, midi, voiced = S.clip([100.0, 110.0, 120.0, 50.0], [0.01, 0.3, 0.02, 0.01], [1.0, 1.0, 1.0, 1e-4])
    assert voiced.tolist() == [True, False, True, False] and confidence == 0.5 and pitch == min(midi[0], midi[2])


def _difference_fp32(x, w, hop, tau_max, fault=None):
    """The kernel's arithmetic in NumPy float32: per term one rounded subtraction and one fma (emulated in float64 and
    rounded: df df + acc with 24-bit factors is exact in float64 up to its own rounding), j ascending."""
    x = np.asarray(x, dtype=np.float32)
    T = S.frames(x.size, w, hop, tau_max)
    d = np.zeros((T, tau_max + 1), dtype=np.float32)
    e = np.zeros(T, dtype=np.float32)
    taus = np.arange(tau_max + 1)
    for t in range(T):
        seg = x[t * hop:t * hop + w + tau_max]
        for j in range(w - 1 if fault == "drop_last" else w):
            df = (seg[j] - seg[j + taus]).astype(np.float32)
            d[t] = (df.astype(np.float64) ** 2 + d[t]).astype(np.float32)
            e[t] = np.float32(np.float64(seg[j]) ** 2 + e[t])
    if fault == "shift":
        d = np.concatenate([d[:, 1:], d[:, -1:]], axis=1)
    return d, e


def _pick_fp32(d32, tau_min, tau_max, thr, fault=None):
    """The pick kernel's arithmetic in NumPy float32 (a sequential fp32 prefix sum)."""
    d32 = np.asarray(d32, dtype=np.float32)
    period = np.empty(d32.shape[0], dtype=np.float32)
    ap = np.empty(d32.shape[0], dtype=np.float32)
    tau_f = np.arange(1, tau_max + 1, dtype=np.float32)
    for t, d in enumerate(d32):
        cs = np.cumsum(d[1:], dtype=np.float32)
        dp = np.ones(tau_max + 1, dtype=np.float32)
        np.divide(d[1:] * tau_f, cs, out=dp[1:], where=cs > 0)
        under = np.flatnonzero(dp[tau_min:tau_max] < np.float32(thr))
        if under.size:
            k = tau_min + int(under[0])
            while fault != "no_descent" and k + 1 < tau_max and dp[k + 1] < dp[k]:
                k += 1
        else:
            k = tau_min + int(np.argmin(dp[tau_min:tau_max]))
        a, b, c = d[k - 1], d[k], d[k + 1]
        v = np.float32(np.float32(a - np.float32(2) * b) + c)
        o = np.float32(np.float32(a - c) / np.float32(np.float32(2) * v)) if v > 0 else np.float32(0)
        period[t] = np.float32(k) + (-o if fault == "flip_vertex" else o)
        ap[t] = dp[k]
    return period, ap


def test_difference_comparison_accepts_fp32_and_rejects_planted_faults():
    w, hop, tau_max = 64, 16, 41
    L = w + tau_max + 3 * hop
    x = (np.random.default_rng(3).random(L) * 2 - 1).astype(np.float32)
    d, e = _difference_fp32(x, w, hop, tau_max)
    share = K.compare_difference(d, e, x, w, hop, tau_max)
    assert 0 < share <= 1
    for fault in ("shift", "drop_last"):
        bad_d, bad_e = _difference_fp32(x, w, hop, tau_max, fault)
        with pytest.raises(AssertionError):
            K.compare_difference(bad_d, bad_e, x, w, hop, tau_max)
    # impulses: bit-exact, and the faults show there too (an impulse on the last window sample of a frame)
    imp = np.zeros(L, dtype=np.float32)
    imp[hop + w - 1] = 1.0
    d, e = _difference_fp32(imp, w, hop, tau_max)
    assert K.compare_difference(d, e, imp, w, hop, tau_max, exact=True) == 0.0
    for fault in ("shift", "drop_last"):
        bad_d, bad_e = _difference_fp32(imp, w, hop, tau_max, fault)
        with pytest.raises(AssertionError):
            K.compare_difference(bad_d, bad_e, imp, w, hop, tau_max, exact=True)


@pytest.fixture(scope="module")
def pick_frames():
    return K.pick_frames()


def test_pick_inputs_bind_the_kernel(pick_frames):
    """The 5 % condition of the GPU test holds for the spec alone, and the inputs reach every branch."""
    d32, kinds = pick_frames
    ref = K.certify(d32, S.TAU_MIN, S.TAU_MAX, S.THR)
    ok = ref["certified"]
    print(f"{(~ok).sum()} of {ok.size} frames uncertified ({(~ok & (kinds == 'tone')).sum()} tones, "
          f"{(~ok & (kinds == 'noise')).sum()} noise, {(~ok & (kinds == 'silence')).sum()} silence)")
    assert 1.0 - ok.mean() <= 0.05
    dp = S.normalise(d32.astype(np.float64))
    fallback = ~(dp[:, S.TAU_MIN:S.TAU_MAX] < np.float32(S.THR)).any(1)
    assert fallback[kinds == "noise"].all() and (ok & fallback).sum() >= 10          # the fallback, certified
    assert not fallback[kinds == "tone"].any()
    first = S.TAU_MIN + np.argmax(dp[:, S.TAU_MIN:S.TAU_MAX] < np.float32(S.THR), axis=1)
    assert ((ref["tau"] > first) & ok & ~fallback).sum() >= 100                       # frames with a descent
    assert (ref["tau"][kinds == "silence"] == S.TAU_MIN).all() and (ref["aperiodicity"][kinds == "silence"] == 1).all()
    assert (np.abs(ref["period"] - ref["tau"])[ok & (kinds == "tone")] > 0.05).sum() >= 100   # vertices off the lag


def test_pick_comparison_accepts_fp32_and_rejects_planted_faults(pick_frames):
    d32, _ = pick_frames
    args = (S.TAU_MIN, S.TAU_MAX, S.THR)
    period, ap = _pick_fp32(d32, *args)
    uncertified, p_share, ap_share = K.compare_pick(period, ap, d32, *args)
    print(f"fp32 model: uncertified {uncertified:.3f}, period err/bound {p_share:.3f}, aperiodicity err/bound {ap_share:.3f}")
    assert p_share <= 1 and ap_share <= 1
    for fault in ("no_descent", "flip_vertex"):
        with pytest.raises(AssertionError):
            K.compare_pick(*_pick_fp32(d32, *args, fault=fault), d32, *args)
    # inputs that cannot bind the kernel are refused as such: silence alone has no certified frame
    with pytest.raises(AssertionError, match="uncertified"):
        K.compare_pick(np.full(4, 8.0), np.ones(4), np.zeros((4, S.TAU_MAX + 1), dtype=np.float32), *args)


def test_frames_and_refusals_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    for L, w, hop, tau_max in ((12000, 3072, 768, 1920), (4992, 3072, 768, 1920), (5759, 3072, 768, 1920),
                               (5760, 3072, 768, 1920), (185, 64, 16, 41), (105, 64, 16, 41), (200, 64, 7, 40)):
        assert lib.isi_pitch_frames(L, w, hop, tau_max) == S.frames(L, w, hop, tau_max) == (L - w - tau_max) // hop + 1
    assert lib.isi_pitch_frames(4992, 3072, 768, 1920) == 1 and lib.isi_pitch_frames(4991, 3072, 768, 1920) == -1
    assert lib.isi_pitch_frames(5000, 0, 768, 1920) == -1 and lib.isi_pitch_frames(5000, 3072, 0, 1920) == -1
    assert lib.isi_pitch_frames(5000, 3072, 768, -1) == -1

    ok = dict(x=FAKE, xs=12000, d=FAKE, e=FAKE, B=1, L=12000, W=3072, hop=768, tau_max=1920)

    def diff(**kw):
        a = dict(ok, **kw)
        return lib.isi_pitch_difference_f32(a["x"], a["xs"], a["d"], a["e"], a["B"], a["L"], a["W"], a["hop"], a["tau_max"], None)
    for name in ("x", "d", "e"):
        assert diff(**{name: None}) == -1 and b"null" in lib.isi_last_error()
    assert diff(B=0) == -1 and diff(L=0) == -1 and diff(W=0) == -1 and diff(hop=0) == -1 and diff(B=-2) == -1
    assert diff(tau_max=2) == -1
    assert diff(L=4991, xs=4991) == -1 and b"shorter than one frame" in lib.isi_last_error()
    assert diff(xs=11999) == -1 and b"stride" in lib.isi_last_error()
    assert diff(x=FAKE + 2) == -1
    assert diff(W=13441, L=1 << 20, xs=1 << 20) == -4 and b"LDS" in lib.isi_last_error()      # W + tau_max = 15361
    assert diff(L=1 << 31, xs=1 << 31) == -4 and b"2^31" in lib.isi_last_error()

    okp = dict(d=FAKE, n=10, tau_min=8, tau_max=1920, thr=0.1, period=FAKE, ap=FAKE)

    def pick(**kw):
        a = dict(okp, **kw)
        return lib.isi_pitch_pick_f32(a["d"], a["n"], a["tau_min"], a["tau_max"], a["thr"], a["period"], a["ap"], None)
    for name in ("d", "period", "ap"):
        assert pick(**{name: None}) == -1 and b"null" in lib.isi_last_error()
    assert pick(n=0) == -1 and pick(n=-1) == -1
    assert pick(tau_min=0) == -1 and b"tau_min" in lib.isi_last_error()
    assert pick(tau_min=8, tau_max=9) == -1 and b"tau_min + 2" in lib.isi_last_error()
    for thr in (float("nan"), 0.0, -0.1, 1.5, float("inf")):
        assert pick(thr=thr) == -1 and b"threshold" in lib.isi_last_error()
    assert pick(tau_max=15360) == -4 and b"LDS" in lib.isi_last_error()
    assert pick(n=1 << 31) == -4

    # no CPU path, and the surfaces exist
    import inpainting
    from GANsynth_pytorch import pitch as PT
    assert (PT.FS_A, PT.W, PT.HOP, PT.TAU_MAX, PT.TAU_MIN, PT.THR, PT.VOICED_AP, PT.VOICED_E) == (
        S.FS_A, S.W, S.HOP, S.TAU_MAX, S.TAU_MIN, S.THR, S.VOICED_AP, S.VOICED_E) == (48000, 3072, 768, 1920, 8, 0.1, 0.2, 1e-3)
    with pytest.raises(_hip.HipLibraryError):
        PT.estimate_pitch(torch.zeros(8000), 16000)
    assert callable(inpainting.estimate_pitch)
