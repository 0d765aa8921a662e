"""Host-side checks of the formant correction (csrc/formant.hip, GANsynth_pytorch/stretch.py and bend.py, inpainting.py, the
routes): the float32 model in the kernel's order stays inside the derived bound of tests/formant_spec.py on every kernel
case; every planted fault of the definition is rejected by the same comparison; the data hold what the cases promise; the
envelope's own properties; `formant_order` by hand; the entry point and the Python calls refuse bad arguments before any
launch; `preserve_formants=False` never reaches the kernel call; and the float64 experiment's orderings.  No GPU needed.

Float64 figures of the experiment (single-frame idealisation, fs 16 kHz, F = 128, f0 = 440 Hz, order 18, 16 iterations),
partial amplitudes against E(rho h f0) in dB rms, corrected | plain:  +3: 1.38 | 3.43   -4: 2.10 | 4.61   +7: 2.09 | 6.57
+12: 1.35 | 9.91;  with one iteration 1.73 / 3.11 / 2.43 (+3 / -4 / +7), with the hard lifter 4.85 / 4.40 / 5.20."""
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import formant_spec as S


@pytest.fixture(scope="module", params=S.KERNEL_F)
def cases(request):
    return S.kernel_cases(request.param)


def test_float32_model_stays_inside_the_bound(cases):
    for case in cases:
        out, env = S.model32(case.Y, case.ratio, case.order, case.iterations, float(case.depth), float(case.max_gain))
        ratio = S.compare(out, env, case)
        print(f"{case.name}: worst error / bound = {ratio:.4f}")


def test_flagship_case_model():
    case = S.flagship_case()
    out, env = S.model32(case.Y, case.ratio, case.order, case.iterations, float(case.depth), float(case.max_gain))
    assert S.compare(out, env, case) <= 1.0


@pytest.mark.parametrize("fault", S.FAULTS)
def test_planted_faults_are_rejected(fault):
    """the faulty definition, evaluated in float64, fails the comparison on at least one case of F = 64 or F = 130"""
    rejected = 0
    for F in (64, 130):
        for case in S.kernel_cases(F):
            bad = S.spec(case.Y, case.ratio, case.order, case.iterations, float(case.depth), float(case.max_gain), fault=fault,
                         bound=False)
            with np.errstate(over="ignore", invalid="ignore"):
                out, env = bad.out.astype(np.float32), bad.env.astype(np.float32)
            try:
                S.compare(out, env, case)
            except AssertionError:
                rejected += 1
    assert rejected > 0, fault


def test_the_data_hold_what_the_cases_promise():
    orders, iterations, forms, frames, rows, Bs, Ts = set(), set(), set(), set(), set(), set(), set()
    for F in S.KERNEL_F:
        assert S.orders(F) == sorted({2, min(F, 7), min(F, 64), min(F, 256)})
        seen_orders, seen_iterations = set(), set()
        for case in S.kernel_cases(F):
            assert case.Y.shape == (case.B, case.T, 2 * F) and case.ratio.shape == (case.ratio_batch, case.T)
            assert case.ratio_batch in (1, case.B) and 2 <= case.order <= min(F, S.MAX_ORDER)
            seen_orders.add(case.order)
            seen_iterations.add(case.iterations)
            forms.add((case.B, case.ratio_batch))
            Bs.add(case.B)
            Ts.add(case.T)
            rows.update(case.ratio_kinds)
            P = S.power32(case.Y)
            for b in range(case.B):
                for t in range(case.T):
                    kind, p = case.frame_kinds[b][t], P[b, t]
                    frames.add(kind)
                    if kind == "silent":
                        assert p.max() == 0
                    elif kind == "nan":
                        assert np.isnan(p).any()
                    elif kind == "inf":
                        assert np.isinf(p).any() and not np.isnan(p).any()
                    else:
                        assert np.isfinite(p).all() and p.max() >= np.finfo(np.float32).tiny        # Pmax is a normal float
                    if kind == "equal":
                        assert (p == p[0]).all()
                    if kind == "loud_bin":
                        assert (p > 0).sum() == 1
                    if kind == "range_200db" and F >= 64:
                        assert 10 * np.log10(p.max() / p.min()) > 190.0
        assert seen_orders == set(S.orders(F)) and seen_iterations == set(S.KERNEL_ITERATIONS)
    assert frames == set(S.FRAME_KINDS) and rows == set(S.RATIO_KINDS)
    assert forms == {(1, 1), (3, 1), (3, 3)} and Bs == set(S.KERNEL_B) and Ts == set(S.KERNEL_T)
    special = S.ratio_row("special", 6, np.random.default_rng(0))
    assert np.isnan(special).sum() == 1 and np.isinf(special).sum() == 2 and {0.0, -1.0, 1e9} <= set(special[np.isfinite(special)].astype(float))
    rho, unit = S.rho_of(np.array([0.0, -1.0, 1e9, np.nan, np.inf, -np.inf, 1.0, 1.5], np.float32))
    assert rho.tolist() == [0.25, 0.25, 4.0, 1.0, 4.0, 0.25, 1.0, 1.5] and unit.tolist() == [False] * 3 + [True] + [False] * 2 + [True, False]
    assert S.flagship_case().F == 2048 and S.flagship_case().order == 256


def test_a_frame_of_equal_magnitudes_has_a_flat_envelope_and_gain_one():
    F = 64
    Y = np.concatenate([np.full(F, 0.75), np.full(F, -1.25)])[None, None].astype(np.float32)
    level = 0.5 * np.log(float(S.power32(Y)[0, 0, 0]))
    for order, iterations in ((2, 1), (7, 3), (64, 16)):
        r = S.spec(Y, np.full((1, 1), 1.5, np.float32), order, iterations)
        assert np.abs(r.env - level).max() < 1e-12 and np.abs(r.gain - 1.0).max() < 1e-12
        out, env = S.model32(Y, np.full((1, 1), 1.5, np.float32), order, iterations)
        assert np.abs(env - level).max() <= r.env_bound.max() and np.abs(out - Y).max() <= r.bound.max()


def test_the_envelope_rests_on_a_comb_s_peaks():
    """One periodic-Hann frame of the experiment's tone (440 Hz, F = 128: a partial every 7.04 bins, order 18).  After 16
    passes the envelope lies within a factor of two in amplitude (6 dB: the tolerance, chosen as the coarsest figure that
    still tells an envelope on the peaks from a smoothed spectrum, whose level is the comb's log-mean) of every spectral peak
    above the floor, from below or above; after one pass -- plain cepstral smoothing -- it misses every one of them by more.
    Measured in float64: the lowest peak sits 3.7 dB above the envelope after 16 passes (2.4 after 32), 18 to 40 dB after one."""
    F, order = 128, 18
    x = S.formant_tone(2 * F, 440.0)
    X = np.fft.rfft(x * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(2 * F) / (2 * F))))[1:]
    Y = np.concatenate([X.real, X.imag])[None, None].astype(np.float32)
    L = np.log(np.abs(X))
    Lx = np.concatenate([L[:1], L])
    peaks = np.array([k for k in range(2, F) if Lx[k] > Lx[k - 1] and Lx[k] >= Lx[k + 1] and Lx[k] > Lx.max() - S.DEPTH + 1.0])
    assert len(peaks) >= 15
    one = np.ones((1, 1), np.float32)
    many, single = S.spec(Y, one, order, 16), S.spec(Y, one, order, 1)
    tolerance = 6.0 * S.DB
    under_many, under_single = (Lx - many.env[0, 0])[peaks], (Lx - single.env[0, 0])[peaks]
    print(f"peaks above the envelope, dB: 16 passes {under_many.max() / S.DB:.2f}, one pass {under_single.min() / S.DB:.2f} .. {under_single.max() / S.DB:.2f}")
    assert (under_many <= tolerance + many.env_bound.max()).all()
    assert (under_single > tolerance).all()


def test_formant_order_by_hand():
    from GANsynth_pytorch.stretch import formant_order
    assert formant_order(16000, 440.0) == 18          # 18.18
    assert formant_order(16000, 110.0) == 73          # 72.7
    assert formant_order(16000, 220.0) == 36
    assert formant_order(16000, 55.0) == 145
    assert formant_order(16000, 20.0) == 256          # 400 -> the cap
    assert formant_order(16000, 4000.0) == 4          # 2 -> the floor
    assert formant_order(48000, 261.6256) == 92       # 91.7
    for bad in ((0, 440.0), (16000, 0.0), (16000, float("nan")), (float("inf"), 440.0), (16000, -1.0)):
        with pytest.raises(ValueError):
            formant_order(*bad)
    assert S.order_for(16000.0, 440.0) == 18


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    a, b, c, d, e = 0x10000, 0x4000000, 0x8000000, 0xC000000, 0x10000000          # aligned, apart, never dereferenced

    def call(Y=a, ratio=b, ratio_batch=1, table=c, out=d, env=e, B=1, T=4, F=64, order=18, iterations=16, depth=9.2, max_gain=4.6):
        return L.isi_formant_shift_f32(Y, ratio, ratio_batch, table, out, env, B, T, F, order, iterations, depth, max_gain, None)

    INVALID, UNSUPPORTED = -1, -4
    for kw in (dict(Y=None), dict(ratio=None), dict(table=None), dict(out=None), dict(Y=a + 2), dict(ratio=b + 1), dict(table=c + 2),
               dict(out=d + 3), dict(env=e + 2), dict(B=0), dict(T=0), dict(F=0), dict(F=1, order=2), dict(order=1), dict(order=65),
               dict(F=1024, order=257), dict(iterations=0), dict(iterations=65), dict(ratio_batch=2), dict(ratio_batch=0),
               dict(B=3, ratio_batch=2), dict(depth=float("nan")), dict(depth=-1.0), dict(depth=float("inf")),
               dict(max_gain=float("nan")), dict(max_gain=-0.5), dict(max_gain=float("inf")), dict(out=a), dict(out=a + 64),
               dict(env=a + 128), dict(env=d)):
        assert call(**kw) == INVALID, kw
        assert L.isi_last_error().startswith(b"formant_shift:"), kw
    for kw in (dict(F=2049), dict(F=4096, order=300), dict(B=1 << 15, T=1 << 14, F=2, order=2), dict(B=1 << 10, T=1 << 10, F=512)):
        assert call(**kw) == UNSUPPORTED, kw
    assert _hip.FORMANT_MAX_ORDER == 256 and _hip.FORMANT_MAX_ITERATIONS == 64 and _hip.STFT_STRETCH_MAX_F == 2048


def test_python_calls_refuse_bad_arguments_before_any_launch(monkeypatch):
    from GANsynth_pytorch import bend as Bd
    from GANsynth_pytorch import stretch as St
    from interactive_spectrogram_inpainting import _hip
    import inpainting
    helper = SimpleNamespace(fs_hz=16000, n_fft=256, hop_length=64, device=None)
    x = torch.zeros(1000)
    Y, r = torch.zeros(1, 4, 128), torch.ones(4)
    with pytest.raises(_hip.HipLibraryError):
        St.formant_shift(Y, r, 18)                                        # CPU tensors
    monkeypatch.setattr(_hip, "require_gpu", lambda t, name: None)
    monkeypatch.setattr(_hip, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library must not be reached")))
    with pytest.raises(_hip.HipLibraryError):
        St.formant_shift(Y.double(), r, 18)
    with pytest.raises(_hip.HipLibraryError):
        St.formant_shift(Y, r.double(), 18)
    for bad in (dict(Y=torch.zeros(4, 128)), dict(Y=torch.zeros(1, 4, 127)), dict(Y=torch.zeros(1, 4, 2)), dict(Y=torch.zeros(1, 0, 128)),
                dict(Y=torch.zeros(1, 4, 4100)), dict(ratio=torch.ones(5)), dict(ratio=torch.ones(2, 4)), dict(ratio=torch.ones(1, 1, 4)),
                dict(order=1), dict(order=65), dict(iterations=0), dict(iterations=65), dict(floor_db=-1.0),
                dict(floor_db=float("nan")), dict(max_gain_db=float("inf")), dict(max_gain_db=-3.0)):
        kw = dict(Y=Y, ratio=r, order=18)
        kw.update(bad)
        with pytest.raises(ValueError):
            St.formant_shift(**kw)
    monkeypatch.undo()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            St.shift_formants(helper, x, bad)
        with pytest.raises(ValueError):
            inpainting.shift_formants_sound(None, helper, x, bad)
    assert St.shift_formants(helper, x, 0) is x and St.shift_formants(helper, x, 0.0) is x
    assert St.transpose(helper, x, 0, preserve_formants=True) is x
    with pytest.raises(ValueError):
        St.shift_formants(helper, torch.zeros(2, 3, 4), 1.0)
    for order in (1, 129, 300):
        with pytest.raises(ValueError):
            St.transpose(helper, x, 3, preserve_formants=True, formant_order=order)
        with pytest.raises(ValueError):
            Bd.bend(helper, x, 1.0, preserve_formants=True, formant_order=order)
        with pytest.raises(ValueError):
            St._envelope_order(helper, x, order, None)
    with pytest.raises(ValueError):
        St.transpose(helper, x, 3, preserve_formants=True, pitch=float("nan"))
    with pytest.raises(ValueError):
        St.transpose(helper, x, 3, formant_order=18)                       # belongs to preserve_formants=True
    with pytest.raises(ValueError):
        Bd.bend(helper, x, 1.0, pitch=69.0)
    assert St._envelope_order(helper, x, None, 69.0) == 18 and St._envelope_order(helper, x, 40, 69.0) == 40
    assert St._envelope_order(helper, x, None, 9.0) == 128                # 8.2 Hz: the cap 256, then F of the helper
    # no CPU path: a valid call on host tensors is refused by the GPU requirement, not computed
    with pytest.raises(_hip.HipLibraryError):
        St.transpose(helper, x, 3, preserve_formants=True, formant_order=18)
    with pytest.raises(_hip.HipLibraryError):
        St.transpose(helper, x, 3, preserve_formants=True)                # the pitch estimate needs the GPU
    with pytest.raises(_hip.HipLibraryError):
        St.shift_formants(helper, x, 2.0, order=18)
    with pytest.raises(_hip.HipLibraryError):
        St.spectral_envelope(helper, x, order=18)
    with pytest.raises(_hip.HipLibraryError):
        Bd.bend(helper, x, 1.0, preserve_formants=True, formant_order=18)


def test_frame_rates_read_the_curve_at_the_frame_centres():
    from GANsynth_pytorch.bend import bend_maps, frame_rates
    L, N, hop = 4096, 256, 64
    r, phi, frames = bend_maps(L, [0.0, 12.0], [0.0, L / 16000.0], 16000, hop, "cpu")
    rho = frame_rates(r, frames, N, hop)
    centre = np.clip(np.round(frames.numpy() * hop + hop - N / 2), 0, L - 1).astype(int)
    assert rho.dtype == torch.float32 and np.array_equal(rho.numpy(), r.numpy()[centre].astype(np.float32))
    assert rho[0] == np.float32(r[0]) and float(rho[-1]) <= float(r[-1])             # clamped to the sound at the start
    const = frame_rates(*bend_maps(L, 3.0, None, 16000, hop, "cpu")[::2], N, hop)
    assert bool((const == np.float32(2.0 ** 0.25)).all())


def test_routes_refuse_bad_arguments_without_the_gpu():
    import flask_server
    helper = SimpleNamespace(fs_hz=16000, n_fft=128, hop_length=32, device=None)
    client = flask_server.create_app(None, None, None, {}, "cpu", spectrograms_helper=helper).test_client()
    wav = flask_server._wav_bytes(torch.zeros(400), 16000)
    post = lambda url: client.post(url, data=dict(audio=(io.BytesIO(wav), 'upload.wav')), content_type='multipart/form-data')   # noqa: E731
    for url in ("/shift-formants", "/shift-formants?semitones=four", "/shift-formants?semitones=nan", "/shift-formants?semitones=inf",
                "/shift-formants?semitones=30", "/transpose-audio?semitones=2&preserve_formants=yes",
                "/transpose-audio?preserve_formants=1", "/bend-audio?flatten=1&preserve_formants=on",
                "/bend-audio?preserve_formants=1"):
        assert post(url).status_code == 400, url
    assert client.post("/shift-formants?semitones=4").status_code == 400                # no upload
    assert client.post("/shift-formants?semitones=4", data=dict(audio=(io.BytesIO(b"nonsense"), 'x.wav')),
                       content_type='multipart/form-data').status_code == 400
    without = flask_server.create_app(None, None, None, {}, "cpu").test_client()
    assert without.post("/shift-formants?semitones=4").status_code == 501


def test_without_preserve_formants_the_kernel_call_is_never_reached(monkeypatch):
    """`transpose`, `time_stretch`, `bend`, `transpose_sound` and `bend_sound` with the new arguments left out pass the
    vocoder's frames straight to the synthesis: with the vocoder and the synthesis stubbed, `formant_shift` must not run"""
    from GANsynth_pytorch import bend as Bd
    from GANsynth_pytorch import resample as Rs
    from GANsynth_pytorch import stretch as St
    from interactive_spectrogram_inpainting import _hip
    import inpainting
    calls = []

    def forbidden(*a, **k):
        raise AssertionError("formant_shift reached without preserve_formants")

    class Helper(SimpleNamespace):
        def _stft(self, x):
            T = (x.shape[1] - self.n_fft) // self.hop_length + 1 + (self.n_fft // self.hop_length - 1)
            return torch.zeros(x.shape[0], T, self.n_fft), T

    helper = Helper(fs_hz=16000, n_fft=256, hop_length=64, device=None)
    monkeypatch.setattr(St, "formant_shift", forbidden)
    monkeypatch.setattr(_hip, "require_gpu", lambda t, name: None)
    monkeypatch.setattr(St, "stft_stretch", lambda X, pos, hop: torch.zeros(X.shape[0], pos.shape[-1], X.shape[2]))
    monkeypatch.setattr(St, "_synthesise", lambda helper, Y, n: calls.append(Y.shape) or torch.zeros(Y.shape[0], n))
    monkeypatch.setattr(Rs, "resample", lambda y, a, b: y)
    monkeypatch.setattr(Bd, "warp", lambda z, pos, cut: torch.zeros(z.shape[0], pos.shape[-1]))
    x = torch.ones(2048)
    assert St.time_stretch(helper, x, 1.5).shape == (3072,)
    assert St.transpose(helper, x, 3).shape == x.shape
    assert St.transpose(helper, x, 3, preserve_formants=False).shape == x.shape
    assert Bd.bend(helper, x, 2.0).shape == x.shape
    assert Bd.vibrato(helper, x, 6.0, 50.0).shape == x.shape and Bd.glide(helper, x, 0.0, 1.0).shape == x.shape
    assert inpainting.transpose_sound(None, helper, x, semitones=2.0, re_encode=False)[0].shape == x.shape
    assert inpainting.bend_sound(None, helper, x, glide=(0.0, 1.0), re_encode=False)[0].shape == x.shape
    assert len(calls) == 8
    # and with it, the same stubs do reach it
    with pytest.raises(AssertionError, match="formant_shift reached"):
        St.transpose(helper, x, 3, preserve_formants=True, formant_order=18)
    with pytest.raises(AssertionError, match="formant_shift reached"):
        Bd.bend(helper, x, 2.0, preserve_formants=True, pitch=69.0)
    with pytest.raises(AssertionError, match="formant_shift reached"):
        Bd.glide(helper, x, 0.0, 1.0, preserve_formants=True, formant_order=18)


# ------------------------------------------------------------------------------------------------------- the experiment
@pytest.mark.parametrize("semitones", (3, -4, 7))
def test_float64_experiment_orderings(semitones):
    corrected, plain, _, _ = S.experiment(440.0, semitones)
    one_pass = S.experiment(440.0, semitones, iterations=1)[0]
    hard = S.experiment(440.0, semitones, hard=True)[0]
    print(f"{semitones:+d} semitones: corrected {corrected:.2f} dB rms, plain {plain:.2f}, one iteration {one_pass:.2f}, hard lifter {hard:.2f}")
    assert corrected <= 0.7 * plain
    assert corrected < one_pass
    assert corrected < hard


def test_float64_experiment_figures_are_the_recorded_ones():
    want = {3: (1.38, 3.43), -4: (2.10, 4.61), 7: (2.09, 6.57), 12: (1.35, 9.91)}
    for semitones, (c, p) in want.items():
        corrected, plain, _, _ = S.experiment(440.0, semitones)
        assert abs(corrected - c) < 0.01 and abs(plain - p) < 0.01
    for f0, c, p in ((110.0, 0.91, 4.46), (220.0, 1.65, 4.53), (440.0, 2.05, 4.44), (880.0, 2.03, 4.10)):
        corrected, plain, _, _ = S.experiment(f0, 4, F=1024)
        assert abs(corrected - c) < 0.01 and abs(plain - p) < 0.01


def test_smoothing_norm_and_the_table():
    for F, n in ((2, 2), (64, 7), (130, 64), (1024, 145)):
        assert 1.0 <= S.smoothing_norm(F, n) < 1.1                                     # the Hann lifter's kernel is almost positive
    t = S.cos_table(130)
    assert t.dtype == np.float32 and t.shape == (260,) and t[0] == 1 and t[130] == -1 and t[65] == 0 and t[195] == 0
    assert np.abs(t.astype(np.float64) - np.cos(np.pi * np.arange(260) / 130)).max() <= S.U
    from GANsynth_pytorch.stretch import _cos_table
    assert np.array_equal(S.bits(_cos_table(130, "cpu").numpy()), S.bits(t))
