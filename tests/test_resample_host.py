"""Host-side checks of the band-limited sample-rate converter (GANsynth_pytorch/resample.py, csrc/resample.hip): the
geometry the library computes is the written specification's (tests/resample_spec.py), the product's coefficient table
is the spec's, the spec itself has the properties a resampler is used for (unit DC gain, a transparent passband, a
stopband below -140 dB), the caps and the argument checks hold before any launch, and the WAV reader moved without
changing.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_spec as S

PAIRS = {(48000, 16000): (3, 1, 203, 409), (44100, 16000): (441, 160, 187, 815), (16000, 44100): (160, 441, 68, 296),
         (16000, 48000): (1, 3, 68, 137), (22050, 16000): (441, 320, 94, 629)}
FAKE = 0x10000      # non-null, 16-byte aligned, never dereferenced on the host


def _lib_geometry(lib, fs_in, fs_out):
    out = [C.c_int(-7) for _ in range(4)]
    rc = lib.isi_resample_geometry(fs_in, fs_out, *[C.byref(v) for v in out])
    return rc, tuple(v.value for v in out)


def test_geometry_of_the_five_pairs_from_spec_and_library():
    from interactive_spectrogram_inpainting import _hip
    from GANsynth_pytorch import resample as R
    lib = _hip.lib()
    for (fs_in, fs_out), want in PAIRS.items():
        assert S.geometry(fs_in, fs_out) == want
        assert _lib_geometry(lib, fs_in, fs_out) == (0, want)
        assert R.geometry(fs_in, fs_out) == want
    assert S.geometry(32000, 48000) == (2, 3, 68, 138) and _lib_geometry(lib, 32000, 48000) == (0, (2, 3, 68, 138))
    for orig, new in ((3, 1), (441, 160), (160, 441), (1, 3), (2, 3)):
        for L in (0, 1, 1000, 1001):
            assert lib.isi_resample_out_len(L, orig, new) == S.out_len(L, orig, new) == -(-L * new // orig)
    assert lib.isi_resample_out_len(1001, 441, 160) == 364 and lib.isi_resample_out_len(1000, 3, 1) == 334
    assert lib.isi_resample_out_len(-1, 3, 1) == -1 and lib.isi_resample_out_len(10, 0, 1) == -1
    assert lib.isi_resample_out_len((1 << 31) - 1, 1, 441) == ((1 << 31) - 1) * 441
    assert lib.isi_resample_geometry(0, 16000, *[C.byref(C.c_int()) for _ in range(4)]) == -1
    assert lib.isi_resample_geometry(16000, -5, *[C.byref(C.c_int()) for _ in range(4)]) == -1
    assert lib.isi_resample_geometry(48000, 16000, None, None, None, None) == -1


@pytest.mark.parametrize("fs_in,fs_out", list(PAIRS) + [(32000, 48000)])
def test_product_table_is_the_specs_to_one_fp32_ulp(fs_in, fs_out):
    """The two evaluations share the formula; their I0 (numpy's Chebyshev fit / the spec's power series) may differ in
    the last float64 bit, which can move the one rounding to fp32 by an ulp."""
    from GANsynth_pytorch import resample as R
    assert (R.Z, R.ROLLOFF, R.BETA) == (S.Z, S.ROLLOFF, S.BETA) == (64, 0.9475937167399596, 14.769656459379492)
    h = R.resample_table(fs_in, fs_out)
    want = S.table64(fs_in, fs_out)
    assert h.dtype == np.float64 and h.shape == want.shape == S.geometry(fs_in, fs_out)[1::2]
    a, b = h.astype(np.float32), S.table32(fs_in, fs_out)
    assert np.abs(a - b).max() <= np.spacing(np.abs(b)).max() and (np.abs(a - b) <= np.spacing(np.abs(b))).all()
    # the clamped taps are tiny, not zero, and not special-cased
    orig, new, width, taps = S.geometry(fs_in, fs_out)
    assert 0 < abs(want[0, 0]) < 1e-20


@pytest.mark.parametrize("fs_in,fs_out", list(PAIRS))
def test_spec_properties(fs_in, fs_out):
    """The fp32-rounded table with float64 sums: DC gain of every phase within 1e-7 of 1; a 1 kHz tone (amplitude 0.5,
    0.25 s, 20 ms ignored at each end) within 1e-7 of the ideal tone at the new rate; for the down-conversions, tones at
    1.12, 1.25 and 1.5 times the lower Nyquist frequency come out below -140 dB re the input.  Measured with this spec:
    DC 2.1e-8 ... 6.2e-8, tone error 0.8e-8 ... 2.6e-8, stopband -144.2 ... -172.7 dB."""
    h = S.table32(fs_in, fs_out).astype(np.float64)
    assert np.abs(h.sum(1) - 1.0).max() <= 1e-7
    n = np.arange(int(0.25 * fs_in))
    edge = int(0.02 * fs_out)
    y = S.resample(0.5 * np.sin(2 * np.pi * 1000.0 * n / fs_in), fs_in, fs_out)
    assert y.shape == (S.out_len(n.size, *S.geometry(fs_in, fs_out)[:2]),)
    ideal = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(y.size) / fs_out)
    assert np.abs(y - ideal)[edge:-edge].max() <= 1e-7
    if fs_out < fs_in:
        for k in (1.12, 1.25, 1.5):
            y = S.resample(0.5 * np.sin(2 * np.pi * (k * fs_out / 2) * n / fs_in), fs_in, fs_out)
            level = 20 * np.log10(np.abs(y[edge:-edge]).max() / 0.5)
            assert level <= -140.0, (k, level)


def test_spec_identity_and_impulse():
    x = np.arange(5.0)
    assert S.resample(x, 16000, 16000) is not None and np.array_equal(S.resample(x, 16000, 16000), x)
    # an impulse at 0 reads out the table: y[q new + r] = h[r][width - q orig]
    orig, new, width, taps = S.geometry(16000, 48000)
    x = np.zeros(10)
    x[0] = 1.0
    y = S.resample(x, 16000, 48000)
    h = S.table32(16000, 48000).astype(np.float64)
    for n_ in range(y.size):
        q, r = divmod(n_, new)
        assert y[n_] == h[r][width - q * orig]


def test_common_rates_are_inside_the_caps_and_44101_is_refused():
    from interactive_spectrogram_inpainting import _hip
    from GANsynth_pytorch import resample as R
    lib = _hip.lib()
    for rate in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000):
        for fs_in, fs_out in ((rate, 16000), (16000, rate)):
            rc, got = _lib_geometry(lib, fs_in, fs_out)
            assert rc == 0 and got == S.geometry(fs_in, fs_out), (fs_in, fs_out)
            orig, new, width, taps = R.geometry(fs_in, fs_out)
            assert taps <= 16384 and new * taps <= 2 ** 22
    rc, got = _lib_geometry(lib, 44101, 16000)
    assert rc == -4 and got == S.geometry(44101, 16000) and b"16384 taps" in lib.isi_last_error()
    with pytest.raises(ValueError, match="16000/44101"):
        R.geometry(44101, 16000)
    with pytest.raises(ValueError, match="16000/44101"):
        R.resample_table(44101, 16000)
    # the second cap on its own: few enough taps, too many phases
    rc, got = _lib_geometry(lib, 16000, 44101)
    assert got[3] <= 16384 and got[1] * got[3] > 2 ** 22 and rc == -4 and b"2^22" in lib.isi_last_error()
    with pytest.raises(ValueError):
        R.geometry(0, 16000)


def test_argument_checks_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    from GANsynth_pytorch import resample as R
    lib = _hip.lib()
    ok = dict(x=FAKE, xs=1000, y=FAKE, ys=334, B=1, L=1000, orig=3, new=1, width=203, table=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.isi_resample_f32(a["x"], a["xs"], a["y"], a["ys"], a["B"], a["L"], a["orig"], a["new"], a["width"],
                                    a["table"], None)
    for name in ("x", "y", "table"):
        assert call(**{name: None}) == -1 and b"null" in lib.isi_last_error()
    assert call(B=0) == -1 and call(L=0) == -1 and call(orig=0) == -1 and call(new=-1) == -1 and call(width=0) == -1
    assert call(xs=999) == -1 and b"stride" in lib.isi_last_error()
    assert call(ys=333) == -1 and b"stride" in lib.isi_last_error()
    assert call(x=FAKE + 2) == -1
    assert call(L=1 << 31, xs=1 << 31, ys=1 << 31) == -4 and b"2^31" in lib.isi_last_error()
    assert call(width=8191, orig=3) == -4 and b"16384 taps" in lib.isi_last_error()          # 16385 taps
    assert call(width=100, orig=441, new=8000, ys=1 << 30) == -4 and b"2^22" in lib.isi_last_error()
    # no CPU path
    with pytest.raises(_hip.HipLibraryError):
        R.resample(torch.zeros(100), 48000, 16000)
    with pytest.raises(_hip.HipLibraryError):
        R.resample(torch.zeros(2, 100), 16000, 16000)
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper, SpectrogramsHelper
    assert MelSpectrogramsHelper.from_wavfile is SpectrogramsHelper.from_wavfile


def test_read_wav_round_trips_and_flask_server_keeps_its_name():
    import flask_server
    from GANsynth_pytorch.wavfile import read_wav
    x = torch.sin(torch.arange(1500) * 0.05) * 0.5
    for rate in (16000, 22050, 48000):
        wav = flask_server._wav_bytes(x, rate)
        got, got_rate = read_wav(wav)
        assert got_rate == rate and got.dtype == torch.float32 and got.shape == (1500,)
        assert torch.equal(got, (x.clamp(-1, 1) * 32767.0).round() / 32768.0)
        again, again_rate = flask_server._read_wav(wav)
        assert again_rate == rate and torch.equal(again, got)
    for bad in (b"nonsense", b"RIFF\x00\x00\x00\x00WAVE"):
        with pytest.raises(ValueError):
            read_wav(bad)
        with pytest.raises(ValueError):
            flask_server._read_wav(bad)
