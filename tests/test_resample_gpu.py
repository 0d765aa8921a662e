"""The sample-rate converter's kernel (csrc/resample.hip, isi_resample_f32) against the float64 specification of
tests/resample_spec.py, and the surfaces built on it (`resample`, `SpectrogramsHelper.from_wavfile`,
`inpainting.analyze_audio(fs_hz=)`, the /analyze-audio and /get-audio routes).

The kernel tests hand the kernel the SPEC's coefficients (rounded once to fp32, tap-major), so they isolate the kernel:
  impulses  every output is exactly the table entry the spec names, or 0 (a single non-zero product sums exactly in any
            order): pins every tap index and both edges;
  noise     |y - spec| <= (taps + 2) 2^-24 sum_i |h[r][i] x[..]| per output: the order-free rounding bound of an fp32 sum
            of `taps` rounded products -- derived, nothing to tune.
            Measured on an MI355X: errors up to 1.2e-6, at most 0.09 of the bound.
Pairs: 48000->16000 (one phase), 44100->16000, 16000->44100, 32000->48000 (orig = 2, the even case)."""
import io
import struct

import numpy as np
import pytest
import torch

import resample_spec as S
from test_prior_gpu import _dev, _models

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 16000), (44100, 16000), (16000, 44100), (32000, 48000)]
LENGTHS = [1, 2, 50, 1000, 1001, 4099]       # 50 < every width; 4099: several tiles at every pair


def _spec_table(fs_in, fs_out, dev):
    """The spec's fp32 table in the kernel's layout: tap-major [taps, new]."""
    return torch.from_numpy(S.table32(fs_in, fs_out).T.copy()).to(dev)


def _run_spec_table(x, fs_in, fs_out):
    from GANsynth_pytorch import resample as R
    orig, new, width, _ = S.geometry(fs_in, fs_out)
    y = R._run(x, orig, new, width, _spec_table(fs_in, fs_out, x.device))
    torch.cuda.synchronize()
    return y


def _view(rows, L, dev, seed):
    """[rows, L] uniform noise in [-1, 1] as a view of a wider tensor: row stride L + 7, first sample 3 floats in."""
    g = torch.Generator().manual_seed(seed)
    wide = (torch.rand(rows, L + 7, generator=g) * 2 - 1).to(dev)
    x = wide[:, 3:3 + L]
    assert x.shape == (rows, L) and (rows == 1 or x.stride(0) == L + 7) and not (rows > 1 and x.is_contiguous())
    return x


@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_impulses_read_out_the_table_bit_exactly(fs_in, fs_out):
    dev = _dev()
    L = 1000
    orig, new, width, taps = S.geometry(fs_in, fs_out)
    h = S.table32(fs_in, fs_out)
    positions = [0, L - 1, 500]
    x = torch.zeros(3, L)
    for b, p in enumerate(positions):
        x[b, p] = 1.0
    y = _run_spec_table(x.to(dev), fs_in, fs_out).cpu().numpy()
    n_out = S.out_len(L, orig, new)
    assert y.shape == (3, n_out)
    n = np.arange(n_out)
    q, r = n // new, n % new
    for b, p in enumerate(positions):
        i = p - q * orig + width
        want = np.where((i >= 0) & (i < taps), h[r, np.clip(i, 0, taps - 1)], np.float32(0))
        assert np.count_nonzero(want) > 0
        assert np.array_equal(y[b], want), f"impulse at {p}: {np.flatnonzero(y[b] != want)[:8]}"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("fs_in,fs_out", PAIRS)
def test_noise_against_the_float64_spec(fs_in, fs_out, L, B):
    dev = _dev()
    orig, new, width, taps = S.geometry(fs_in, fs_out)
    x = _view(B, L, dev, seed=L * 7 + B)
    y = _run_spec_table(x, fs_in, fs_out).cpu().numpy().astype(np.float64)
    want, scale = S.resample(x.cpu().numpy(), fs_in, fs_out, with_abs=True)
    assert y.shape == want.shape == (B, -(-L * new // orig))
    bound = (taps + 2) * 2.0 ** -24 * scale
    err = np.abs(y - want)
    print(f"{fs_in}->{fs_out} L={L} B={B}: max err {err.max():.3e}, least bound {bound.min():.3e}, "
          f"max err/bound {(err / np.maximum(bound, 1e-300)).max():.3e}")
    assert (err <= bound).all(), f"{np.argwhere(err > bound)[:8].tolist()}"


def test_output_lengths_batch_invariance_and_identity():
    from GANsynth_pytorch import resample as R
    dev = _dev()
    for (fs_in, fs_out) in PAIRS:
        orig, new, _, _ = S.geometry(fs_in, fs_out)
        for L in LENGTHS:
            x = _view(3, L, dev, seed=L)
            y = R.resample(x, fs_in, fs_out)
            assert y.shape == (3, -(-L * new // orig)) and y.dtype == torch.float32 and y.device == x.device
            # a row of the batch is bit-equal to the same row alone (1-D, and as a one-row batch)
            for b in range(3):
                one = R.resample(x[b], fs_in, fs_out)
                assert one.shape == y.shape[1:] and torch.equal(one, y[b])
            assert torch.equal(R.resample(x[1:2], fs_in, fs_out), y[1:2])
            assert torch.equal(R.resample(x.contiguous(), fs_in, fs_out), y)
    assert R.resample(torch.zeros(1001, device=dev), 44100, 16000).shape == (364,)
    # the public entry (the product's own table) against the spec, and the table cache
    x = _view(2, 1001, dev, seed=4)
    want, scale = S.resample(x.cpu().numpy(), 44100, 16000, with_abs=True)
    got = R.resample(x, 44100, 16000).cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= ((815 + 2) * 2.0 ** -24 + 2.0 ** -23) * scale).all()   # + an ulp on every coefficient
    assert (441, 160, dev) in R._tables and R._tables[(441, 160, dev)].shape == (815, 160)
    # identity: the input itself
    x = _view(2, 50, dev, seed=1)
    assert R.resample(x, 16000, 16000) is x and torch.equal(R.resample(x, 48000, 48000), x)
    assert R.resample(torch.zeros(0, device=dev), 48000, 16000).shape == (0,)
    # a transposed view (no unit stride along the samples) is taken too
    xt = torch.rand(300, 2, generator=torch.Generator().manual_seed(2)).to(dev).t()
    assert torch.equal(R.resample(xt, 48000, 16000), R.resample(xt.contiguous(), 48000, 16000))


@pytest.mark.parametrize("mel", [False, True])
def test_from_wavfile(tmp_path, mel):
    import flask_server
    from GANsynth_pytorch.resample import resample
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper, SpectrogramsHelper
    from GANsynth_pytorch.wavfile import read_wav
    dev = _dev()
    helper = (MelSpectrogramsHelper if mel else SpectrogramsHelper)(16000, 256, 64, 256).to(dev)
    wav = flask_server._wav_bytes(torch.sin(torch.arange(3000) * 0.07) * 0.4, 22050)
    path = tmp_path / "note.wav"
    path.write_bytes(wav)
    x, rate = read_wav(wav)
    assert rate == 22050
    y = resample(x.to(dev), 22050, 16000)
    assert y.shape == (-(-3000 * 320 // 441),)                     # 2177
    for duration_n in (4096, 1024, None):
        spec = helper.from_wavfile(path, duration_n) if duration_n else helper.from_wavfile(str(path))
        n = duration_n or y.numel()
        padded = torch.nn.functional.pad(y, (0, max(0, n - y.numel())))[:n]
        want = helper.to_spectrogram(padded.unsqueeze(0))
        assert spec.shape == (1, 2, 128, -(-n // 64)) and spec.device == want.device and spec.is_cuda
        assert torch.equal(spec, want)


def _app(golden_dir):
    import flask_server
    from GANsynth_pytorch.spectrograms_helper import SpectrogramsHelper
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    _, top, bottom = _models(golden_dir)
    dev = _dev()

    class Enc:                                   # stands in for sklearn's LabelEncoder
        def __init__(self, classes):
            self.classes = list(classes)

        def transform(self, values):
            return np.array([self.classes.index(v) for v in values])
    encoders = {"pitch": Enc(range(24, 85)), "instrument_family_str": Enc([f"fam{i}" for i in range(11)])}
    torch.manual_seed(9)
    vq = VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
               num_embeddings=64, resolution_factors={"bottom": 4, "top": 2}).to(dev).eval()
    helper = SpectrogramsHelper(16000, 128, 32, 128).to(dev)
    app = flask_server.create_app(vq, top, bottom, encoders, dev, spectrograms_helper=helper, top_p=0.9, seed=0)
    return app.test_client(), vq, top, bottom, helper, dev


def _upload(client, wav):
    return client.post("/analyze-audio?pitch=64&instrument_family_str=fam2", data={"audio": (io.BytesIO(wav), "note.wav")},
                       content_type="multipart/form-data")


def test_routes(golden_dir):
    import json
    import flask_server
    import inpainting
    from GANsynth_pytorch.resample import resample
    c, vq, top, bottom, helper, dev = _app(golden_dir)
    # a 48 kHz upload: converted to the models' rate, then the flow of a 16 kHz one
    wav = flask_server._wav_bytes(torch.sin(torch.arange(4500) * 0.017) * 0.5, 48000)
    r = _upload(c, wav)
    assert r.status_code == 200
    body = r.get_json()
    x, rate = flask_server._read_wav(wav)
    assert rate == 48000 and x.numel() == 4500
    y = resample(x.to(dev), 48000, 16000)
    assert y.numel() == 1500
    res_n = inpainting.top_resolution_n(vq, top, bottom, helper, dev)
    dur = inpainting.adapt_duration(y.numel(), 16000, 4.0, res_n, 4)
    assert dur == 6 * res_n
    t, b = inpainting.analyze_audio(vq, helper, y, dur, dev)
    assert np.array(body["top_code"]).shape == (8, 6) and np.array(body["bottom_code"]).shape == (16, 12)
    assert t[0].cpu().tolist() == body["top_code"] and b[0].cpu().tolist() == body["bottom_code"]
    assert body["top_conditioning"]["pitch"][0][0] == 64
    # the library call resamples by itself when told the rate; the default is today's behaviour
    t2, b2 = inpainting.analyze_audio(vq, helper, x, dur, dev, fs_hz=48000)
    assert torch.equal(t2, t) and torch.equal(b2, b)
    t3, b3 = inpainting.analyze_audio(vq, helper, y, dur, dev, fs_hz=16000)
    assert torch.equal(t3, t) and torch.equal(b3, b)
    # an upload longer than the service keeps: cut before the copy, same codes as the whole file trimmed afterwards
    g = torch.Generator().manual_seed(3)
    long = (torch.rand(4 * 48000 + 5000, generator=g) - 0.5)
    wav_long = flask_server._wav_bytes(long, 48000)
    r_long = _upload(c, wav_long)
    assert r_long.status_code == 200
    xl, _ = flask_server._read_wav(wav_long)
    tl, bl = inpainting.analyze_audio(vq, helper, xl, 64000, dev, fs_hz=48000)
    assert tl[0].cpu().tolist() == r_long.get_json()["top_code"] and bl[0].cpu().tolist() == r_long.get_json()["bottom_code"]
    # a ratio beyond the caps: 400 with the reason
    bad = _upload(c, flask_server._wav_bytes(torch.zeros(2000), 44101))
    assert bad.status_code == 400 and b"16000/44101" in bad.data
    # /get-audio: byte-identical without the argument, resampled with it
    codes = json.dumps({"top_code": body["top_code"], "bottom_code": body["bottom_code"]})
    plain = c.post("/get-audio", data=codes)
    assert plain.status_code == 200 and plain.mimetype == "audio/wav"
    audio = inpainting.codes_to_audio(vq, helper, t, b)[0]
    n = audio.numel()
    assert n == 6 * res_n
    pcm = (audio.clamp(-1, 1) * 32767.0).round().to(torch.int16).cpu().numpy().tobytes()
    header = b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVEfmt " + struct.pack(
        "<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + struct.pack("<I", len(pcm))
    assert plain.data == header + pcm
    up = c.post("/get-audio?fs_hz=48000", data=codes)
    assert up.status_code == 200 and up.mimetype == "audio/wav"
    assert struct.unpack("<I", up.data[24:28])[0] == 48000 and struct.unpack("<I", up.data[28:32])[0] == 96000
    assert len(up.data) - 44 == 2 * -(-3 * n // 1) and struct.unpack("<I", up.data[40:44])[0] == 2 * 3 * n
    x_up, rate_up = flask_server._read_wav(up.data)
    assert rate_up == 48000
    want = (resample(audio, 16000, 48000).clamp(-1, 1) * 32767.0).round() / 32768.0
    assert torch.equal(x_up, want.cpu())
    assert c.post("/get-audio?fs_hz=16000", data=codes).data == plain.data
    assert c.post("/get-audio?fs_hz=44101", data=codes).status_code == 400
