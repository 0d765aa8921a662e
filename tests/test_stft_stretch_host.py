"""The phase-locked stretch without a GPU: the float32 model of isi_stft_stretch_f32 inside the bound of the float64
specification (tests/stft_stretch_spec.py) on every kernel case, the comparison against planted faults, properties of the
specification and of the host side of GANsynth_pytorch.stretch, every refusal of the C entry (the library loads without a GPU
and refuses before any launch), the routes' refusals, and the float64 experiment behind the method.

Figures of the experiment (n_fft 256, hop 64, 16 kHz, 64 frames, three decaying partials of 440 Hz with a 10 ms attack;
spectral convergence against the ideally stretched sound):
    factor 0.75: locked 0.038, plain vocoder 0.072        factor 1.5: locked 0.047, plain 0.261
    factor 2.0:  locked 0.062, plain 0.631 (its rms falls to 0.38 of the ideal's; the locked one's is 0.998)
    factor 3.0:  locked 0.090, plain 0.247
    +3 semitones (44/37): 0.025 against the untransposed sound's 1.07;  -4 semitones (277/349): 0.034 against 1.11"""
import io
import math

import numpy as np
import pytest
import torch

import stft_stretch_spec as S

PI = math.pi


@pytest.fixture(scope="module")
def cases():
    return [c for T in S.KERNEL_T for F in S.KERNEL_F for c in S.kernel_cases(T, F)]


# ------------------------------------------------------------------------------------------- the model, the comparison
def test_float32_model_stays_inside_the_bound_on_every_kernel_case(cases):
    worst = max(S.compare(S.stretch(c.X, c.pos, c.hop, np.float32).out, c) for c in cases)
    print(f"{len(cases)} cases, worst error / bound of the float32 model: {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_comparison_rejects_planted_faults(cases, mutant):
    rejected = 0
    for c in cases:
        if c.F < 64 or c.T < 17:
            continue
        try:
            S.compare(S.stretch(c.X, c.pos, c.hop, np.float32, mutant).out, c, mutant)
        except AssertionError:
            rejected += 1
    print(f"{mutant}: rejected on {rejected} cases")
    assert rejected >= 1


def test_the_data_hold_what_the_cases_promise(cases):
    seen = set()
    for c in cases:
        src = c.spec.src
        assert float(src.margin.min()) >= S.WRAP_MARGIN if src.margin.size else True
        P = S.power(c.X)
        runs = [S.copy_run(c.pos[r], c.T) for r in range(c.pos_batch)]
        seen |= {"copy 0"} if 0 in runs else set()
        seen |= {"copy 1"} if 1 in runs else set()
        seen |= {"copy all"} if c.T_out in runs and c.T_out > 1 else set()
        seen |= {"silent frame"} if (P == 0).all(-1).any() else set()
        seen |= {"tie"} if src.tie.any() else set()
        seen |= {"equal magnitudes"} if ((P == P[..., :1]).all(-1) & (P[..., 0] > 0)).any() and c.F > 1 else set()
        seen |= {"peak at 0"} if src.peak[..., 0].any() else set()
        seen |= {"peak at F - 1"} if src.peak[..., -1].any() and c.F > 2 else set()
        seen |= {"plateau"} if c.F >= 12 and (src.peak[..., c.F // 2] & (P[..., c.F // 2] == P[..., c.F // 2 + 1])).any() else set()
        with np.errstate(invalid="ignore"):
            seen |= {"frozen"} if c.T_out > 2 and (np.diff(c.pos, axis=1) == 0).all(1).any() else set()
            seen |= {"decreasing"} if c.T_out > 2 and (np.diff(c.pos, axis=1) < 0).all(1).any() else set()
            seen |= {"below 0"} if (c.pos < 0).any() else set()
            seen |= {"above T - 1"} if (c.pos > c.T - 1).any() else set()
        seen |= {"nan"} if np.isnan(c.pos).any() else set()
        if c.T >= 17 and c.F >= 64:
            moving = np.argmax(P, -1)
            seen |= {"moving peak"} if (np.diff(moving, axis=1) == 1).any() else set()
    assert seen == {"copy 0", "copy 1", "copy all", "silent frame", "tie", "equal magnitudes", "peak at 0", "peak at F - 1", "plateau",
                    "frozen", "decreasing", "below 0", "above T - 1", "nan", "moving peak"}, seen


def test_peaks_and_near_by_hand():
    P = np.array([[0, 3, 3, 1, 0, 2, 0, 0, 5], [1, 1, 1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.float32)
    peak, near, tie = S.peaks_and_near(P.copy())
    assert np.nonzero(peak[0])[0].tolist() == [1, 5, 8]          # bin 2 ties with bin 1 on its left: not a peak; bin 1 is (>=)
    assert near[0].tolist() == [1, 1, 1, 1, 5, 5, 5, 8, 8] and np.nonzero(tie[0])[0].tolist() == [3]   # bin 3: 1 and 5, the lower
    assert S.peaks_and_near(P.copy(), tie_to_upper=True)[1][0].tolist() == [1, 1, 1, 5, 5, 5, 5, 8, 8]
    assert np.nonzero(peak[1])[0].tolist() == [0] and (near[1] == 0).all()           # equal magnitudes: bin 0 alone
    assert not peak[2].any() and near[2].tolist() == list(range(9))                  # silence: every bin follows itself


def test_rate_one_positions_are_the_identity_bit_for_bit(cases):
    for c in cases[::7]:
        pos = np.arange(c.T, dtype=np.float32)[None]
        for dtype in (np.float64, np.float32):
            s = S.stretch(c.X, pos, c.hop, dtype)
            if dtype == np.float32:
                assert np.array_equal(S.bits(s.out), S.bits(c.X))
            else:
                assert s.copied.all() and np.array_equal(S.bits(s.raw), S.bits(c.X)) and (s.bound == 0).all()


def test_copy_run_agrees_with_the_formula_in_exact_arithmetic():
    """The rule only fixes the bits.  The formula on whole positions p, p + 1, ...: f == 0, so M = A[t] and, by induction,
    Phi'[n] + Omega_n + dev[t-1, n] = phi[t, n] modulo 2 pi, hence Phi[j] = phi[t, j].  What is left in float64 is the float32
    rounding of P (A is its root): 2u relative."""
    source = S.make_source(3, 17, 64)
    pos = np.arange(17, dtype=np.float32)[None]
    spec = S.stretch(source.X, pos, source.hop)
    free = S.stretch(source.X, pos, source.hop, copy=False)
    assert spec.copied.all() and not free.copied.any()
    assert (np.abs(free.out - spec.out) <= 3 * S.U * np.abs(spec.out) + 1e-12).all()


# ----------------------------------------------------------------------------------------- GANsynth_pytorch.stretch, host
def test_stretch_positions():
    from GANsynth_pytorch.stretch import stretch_positions
    p = stretch_positions(125, factor=1)
    assert p.dtype == torch.float32 and torch.equal(p, torch.arange(125, dtype=torch.float32))
    assert torch.equal(stretch_positions(40, factor=1.0, keep_head=5, keep_tail=7), torch.arange(40, dtype=torch.float32))
    p = stretch_positions(40, factor=2.0, keep_head=5, keep_tail=7)
    assert p.numel() == 80
    assert torch.equal(p[:5], torch.arange(5.0)) and torch.equal(p[-7:], torch.arange(33.0, 40.0))    # head and tail at rate 1
    middle = p[5:-7].double()
    assert middle[0] == 5 and torch.allclose(middle.diff(), torch.full((67,), 28 / 68, dtype=torch.float64), atol=1e-5)
    assert float(middle[-1]) < 33 and (p.diff() > 0).all()
    assert np.array_equal(p.numpy(), S.positions(40, factor=2.0, keep_head=5, keep_tail=7))
    assert stretch_positions(10, factor=0.04).numel() == 1
    assert np.allclose(stretch_positions(10, n_out=3).numpy(), [0.0, 10 / 3, 20 / 3])
    for bad in (dict(factor=0.0), dict(factor=-1.0), dict(factor=float("nan")), dict(factor=float("inf")), dict(),
                dict(factor=1.0, n_out=10), dict(factor=1.0, keep_head=6, keep_tail=5), dict(factor=0.5, keep_head=3, keep_tail=3),
                dict(factor=1.0, keep_head=-1), dict(n_out=0), dict(factor=2.0, keep_head=5, keep_tail=5)):
        with pytest.raises(ValueError):
            stretch_positions(10, **bad)


def test_transpose_ratio():
    from GANsynth_pytorch.stretch import transpose_ratio
    try:
        from interactive_spectrogram_inpainting import _hip
        _hip.lib()
        built = True
    except Exception:                                                        # the library is not built
        built = False
    if built:
        assert transpose_ratio(0) == (1, 1, 0.0)
        assert transpose_ratio(12)[:2] == (2, 1) and transpose_ratio(-12)[:2] == (1, 2)
        for s in list(range(-12, 0)) + list(range(1, 13)) + [0.5, -2.25]:
            num, den, cents = transpose_ratio(s)
            assert math.gcd(num, den) == 1 and den <= 512
            assert abs(1200 * math.log2(num / den) - 100 * s - cents) < 1e-9
            assert abs(cents) < 0.1, (s, num, den, cents)
        assert transpose_ratio(7, max_denominator=2)[:2] == (3, 2)
    with pytest.raises(ValueError):
        transpose_ratio(float("nan"))


def test_stft_stretch_and_time_stretch_refuse_cpu_tensors_and_bad_shapes():
    from GANsynth_pytorch import stretch
    from GANsynth_pytorch.spectrograms_helper import SpectrogramsHelper
    from interactive_spectrogram_inpainting._hip import HipLibraryError
    helper = SpectrogramsHelper(fs_hz=16000, n_fft=128, hop_length=32, window_length=128)
    with pytest.raises(HipLibraryError):
        stretch.stft_stretch(torch.zeros(1, 4, 8), torch.zeros(3), 2)
    with pytest.raises(HipLibraryError):
        stretch.time_stretch(helper, torch.zeros(640), 2.0)
    with pytest.raises(HipLibraryError):
        helper.to_audio_stretched(torch.zeros(1, 2, 64, 8), torch.arange(8.0))


def test_routes_refuse_without_touching_the_gpu():
    import flask_server
    from GANsynth_pytorch.spectrograms_helper import SpectrogramsHelper
    helper = SpectrogramsHelper(fs_hz=16000, n_fft=128, hop_length=32, window_length=128)
    wav = flask_server._wav_bytes(torch.sin(torch.arange(640) * 0.1) * 0.5, 16000)
    client = flask_server.create_app(None, None, None, {}, "cpu", spectrograms_helper=helper).test_client()
    post = lambda url, **data: client.post(url, data=data, content_type='multipart/form-data')   # noqa: E731
    audio = lambda: (io.BytesIO(wav), 'a.wav')                                                   # noqa: E731
    assert post('/transpose-audio?semitones=3').status_code == 400                        # no audio part
    assert post('/transpose-audio?semitones=3', audio=(io.BytesIO(b"not a wave file"), 'a.wav')).status_code == 400
    assert post('/transpose-audio', audio=audio()).status_code == 400                     # neither argument
    assert post('/transpose-audio?semitones=3&to_pitch=60', audio=audio()).status_code == 400
    assert post('/transpose-audio?semitones=high', audio=audio()).status_code == 400
    assert post('/transpose-audio', audio=audio(), semitones='nan').status_code == 400    # a form field, not finite
    assert post('/stretch-audio', audio=audio()).status_code == 400                       # no factor
    assert post('/stretch-audio?factor=2').status_code == 400
    for query in ('factor=0', 'factor=-2', 'factor=nan', 'factor=x', 'factor=2&keep_attack_s=-1', 'factor=2&keep_attack_s=1&keep_release_s=1'):
        assert post('/stretch-audio?' + query, audio=audio()).status_code == 400, query
    assert client.get('/transpose-audio').status_code == 405 and client.get('/stretch-audio').status_code == 405
    no_helper = flask_server.create_app(None, None, None, {}, "cpu").test_client()
    for url in ('/transpose-audio?semitones=3', '/stretch-audio?factor=2'):
        assert no_helper.post(url, data={'audio': audio()}, content_type='multipart/form-data').status_code == 501


# ------------------------------------------------------------------------------------------ refusals before any launch
def test_entry_point_refuses_bad_arguments_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    ok = 0x10000                     # non-null, never dereferenced on the host
    INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
    good = dict(X=ok, pos=ok, pos_batch=1, out=ok, ws=ok, ws_bytes=None, B=2, T=5, T_out=9, F=3, hop=2)

    def call(**change):
        g = dict(good, **change)
        if g["ws_bytes"] is None:
            g["ws_bytes"] = 1 << 62
        return L.isi_stft_stretch_f32(g["X"], g["pos"], g["pos_batch"], g["out"], g["ws"], g["ws_bytes"], g["B"], g["T"], g["T_out"],
                                      g["F"], g["hop"], None)

    def refused(rc, message, code=INVALID):
        assert rc == code
        assert message in L.isi_last_error(), L.isi_last_error()

    for name in ("X", "pos", "out", "ws"):
        refused(call(**{name: None}), b"stft_stretch: null pointer")
    for name in ("B", "F", "T_out"):
        for v in (0, -1):
            refused(call(**{name: v}), b"stft_stretch: B, F and T_out must be at least 1")
    for v in (1, 0, -3):
        refused(call(T=v), b"stft_stretch: T must be at least 2")
    for v in (0, 3, -1):
        refused(call(pos_batch=v), b"stft_stretch: pos_batch must be 1 or B")
    for v in (0, -2, 4, 12):
        refused(call(hop=v), b"stft_stretch: hop must be positive and divide n_fft")
    refused(call(ws=ok + 2), b"stft_stretch: workspace must be aligned")
    cap = 2048                                                                            # ISI_STFT_STRETCH_MAX_F
    refused(call(F=cap + 1, hop=1), b"stft_stretch: F above ISI_STFT_STRETCH_MAX_F", UNSUPPORTED)
    span = b"stft_stretch: T must stay at or below 2^24"
    refused(call(B=1, T=(1 << 24) + 1, F=1, hop=1), span, UNSUPPORTED)
    refused(call(B=1, T=1 << 19, F=1 << 10, hop=1), span, UNSUPPORTED)                    # X: exactly 2^30 elements
    refused(call(B=1 << 10, pos_batch=1, T=2, T_out=1 << 9, F=1 << 10, hop=1), span, UNSUPPORTED)   # out: 2^30
    assert L.isi_stft_stretch_workspace_bytes(2, 5, 3) == 4 * 4 * 2 * 5 * 3
    assert L.isi_stft_stretch_workspace_bytes(1, 125, 1024) == 16 * 125 * 1024            # the flagship size runs
    for bad in ((0, 5, 3), (2, 1, 3), (2, 5, 0), (2, 5, cap + 1), (1 << 10, 1 << 10, 1 << 10)):
        assert L.isi_stft_stretch_workspace_bytes(*bad) == 0
    refused(call(ws_bytes=4 * 4 * 2 * 5 * 3 - 1), b"stft_stretch: workspace_bytes 479 < 480", WORKSPACE)


# ------------------------------------------------------------------------------------------------------ the experiment
def test_locked_stretch_against_the_plain_vocoder():
    figures = {}
    for factor in (0.75, 1.5, 2.0, 3.0):
        locked, plain, rms_locked, rms_plain = S.experiment_stretch(factor)
        figures[factor] = (locked, plain)
        print(f"factor {factor}: locked {locked:.3f}, plain vocoder {plain:.3f}; rms against the ideal's {rms_locked:.3f}, {rms_plain:.3f}")
        assert locked < plain
    for factor in (1.5, 2.0):
        assert figures[factor][0] <= figures[factor][1] / 2


@pytest.mark.parametrize("semitones, ratio", [(3, (44, 37)), (-4, (277, 349))])
def test_transposition_against_the_partials_at_the_new_pitch(semitones, ratio):
    assert abs(1200 * math.log2(ratio[0] / ratio[1]) - 100 * semitones) < 0.05
    transposed, untransposed = S.experiment_transpose(semitones, *ratio)
    print(f"{semitones:+d} semitones ({ratio[0]}/{ratio[1]}): {transposed:.3f} against the untransposed sound's {untransposed:.3f}")
    assert transposed <= untransposed / 10
