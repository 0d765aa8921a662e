"""The kernels of csrc/spectrogram.hip, one by one through the C-ABI, against the float64 specifications of
tests/spectrogram_spec.py: polar / unwrap, finish / transpose, inverse-prepare scan, polar-to-rectangular, overlap-add, the two
adjoints, the two spectral-distance kernels and the affine / mask kernel.  Every kernel is handed its own float32 input, so no
element is excluded from any comparison: the input conditions that make this possible (every wrapped difference at least
0.01 rad from an odd multiple of pi, no sign or mask decision within rounding of its threshold) are asserted from the float64
spec alone.  Inputs and outputs lie inside NaN buffers with 64-float guards: a read outside an input brings NaN into the
result, and the guards of every output must keep their bits.

Rules (tests/spectrogram_spec.py holds them, tests/test_spectrogram_kernels_host.py shows what they accept and reject):
  element-wise outputs and the float32-conditioned sums: tests_support.compare_rows against the float32 yardstick, margin 8,
  floor 2^-23; the running sums and the overlap-add: the derived order-free bounds; impulses, pinned sums, masks, padding and
  untouched samples: exact.

Largest measured ratio per kernel on the MI355X (profiles/spectrogram_checks.txt).  compare_rows: error / float32 yardstick,
at most 8; derived bound: error / bound, at most 1:
  spec_polar_kernel                 compare_rows 1.64 (a, mel 0); the mel running phase 1.36
  spec_finish_kernel                compare_rows 1.41; the wrap-end case 0.20 of 2^-20 on the circle
  spec_inverse_prepare_kernel       exp(ch0) 0.57; running sum 0.53 of its bound (the sequential float32 scan on the CPU reaches
                                    the same 0.53 on that case, B = 3, T = 2, F = 70)
  spec_to_stft_kernel               compare_rows 4.30 (mel, B = 3, T = 65, F = 1: rows of two elements); 1.82 on every other case
  overlap_add_kernel                0.39 of its bound; impulses and untouched samples exact
  spec_to_stft_bwd_kernel           compare_rows 2.42
  spec_inverse_prepare_bwd_kernel   d ch0 0.85; reverse running sum 0.51 of its bound
  spec_distance_fwd_kernel          compare_rows 1.09; pinned sums exact
  spec_distance_bwd_kernel          compare_rows 2.07; padding and the zero-magnitude bins exact
  spec_affine_mask_kernel           compare_rows 0.44; the mask bit-exact

A recording aid, not a check: with ISI_SPEC_RECORD=<file> in the environment every comparison's error, yardstick or bound and
ratio are written there when the module ends, worst first, with the module's wall time.
"""
import ctypes as C
import os
import time

import pytest
import torch

import spectrogram_spec as SP
from test_conv_wgrad_gpu import Out
from test_prior_gpu import _dev

pytestmark = pytest.mark.gpu

RECORD = []                    # spectrogram_spec.Check of every comparison


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    t0 = time.time()
    yield
    path = os.environ.get("ISI_SPEC_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# kernel error, its yardstick (floored at 2^-23; rule: ratio <= 8, tests_support.compare_rows) or derived bound (rule:\n"
                "# ratio <= 1) and their ratio against the float64 spec, per comparison of tests/test_spectrogram_kernels_gpu.py.\n"
                "# Case names: B-T-F-mel, B-T-F (scans), nfft-hop-left-T-L-B (overlap_add), B-T-F-RS-rows_per_block (distance_fwd),\n"
                "# B-T-F-RS-kind (distance_bwd), B-HW-ref-mask (affine_mask).\n"
                f"# Worst ratio first.  Wall time of the file, reference computations on the CPU included: {time.time() - t0:.1f} s\n")
        worst = {}
        for c in RECORD:
            key = (c.kernel, c.rule)
            worst[key] = max(worst.get(key, 0.0), c.ratio)
        for (kernel, rule), r in sorted(worst.items()):
            f.write(f"# largest ratio, {kernel} ({'derived bound, <= 1' if rule == 'bound' else 'compare_rows, <= 8'}): {r:.3f}\n")
        for c in sorted(RECORD, key=lambda c: -c.ratio):
            f.write(f"{c.ratio:8.3f}  err {c.err:.3e}  {'bound    ' if c.rule == 'bound' else 'yardstick'} {c.bound:.3e}  {c.kernel} {c.case} {c.what}\n")


def _in(t, dev):
    """A float32 input inside a NaN buffer."""
    o = Out(tuple(t.shape), dev)
    o.view.copy_(t)
    o.bits = o.buf.view(torch.int32).clone()
    return o


def _run(name, *args):
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    rc = getattr(L, name)(*args, None)
    assert rc == 0, L.isi_last_error()
    torch.cuda.synchronize()


def _p(o):
    return o.view.data_ptr()


def _intact(*bufs):
    assert all(b.intact() for b in bufs), "a write outside an output (or into an input's guard)"


@pytest.mark.parametrize("case", SP.POLAR_CASES, ids=SP.case_id)
def test_polar(case):
    (B, T, F), mel = case
    dev = _dev()
    x = _in(SP.polar_data(case), dev)
    a, ph = Out((B, T, F), dev), Out((B, T, F), dev)
    _run("isi_spec_polar_f32", _p(x), _p(a), _p(ph), B, T, F, mel)
    _intact(x, a, ph)
    SP.check_polar(case, a.view.cpu(), ph.view.cpu(), RECORD)


@pytest.mark.parametrize("case", SP.TILED_MEL_CASES, ids=SP.case_id)
def test_finish(case):
    (B, T, F), mel = case
    dev = _dev()
    a, ph = (_in(t, dev) for t in SP.finish_data(case))
    out = Out((B, 2, F, T), dev)
    _run("isi_spec_finish_f32", _p(a), _p(ph), _p(out), B, T, F, mel)
    _intact(a, ph, out)
    SP.check_finish(case, out.view.cpu(), RECORD)


def test_finish_wrap_ends():
    dev = _dev()
    a, ph, _ = SP.wrap_end_data()
    a, ph = _in(a, dev), _in(ph, dev)
    out = Out((1, 2, 3, 8), dev)
    _run("isi_spec_finish_f32", _p(a), _p(ph), _p(out), 1, 8, 3, 0)
    _intact(a, ph, out)
    SP.check_finish_wrap_ends(out.view.cpu(), RECORD)


@pytest.mark.parametrize("shape", SP.SCAN_CASES, ids=SP.case_id)
def test_inverse_prepare(shape):
    B, T, F = shape
    dev = _dev()
    spec = _in(SP.spec_data(shape), dev)
    a, ph = Out((B, T, F), dev), Out((B, T, F), dev)
    _run("isi_spec_inverse_prepare_f32", _p(spec), _p(a), _p(ph), B, T, F)
    _intact(spec, a, ph)
    SP.check_inverse_prepare(shape, a.view.cpu(), ph.view.cpu(), RECORD)


@pytest.mark.parametrize("shape", SP.SCAN_CASES, ids=SP.case_id)
def test_inverse_prepare_bwd(shape):
    B, T, F = shape
    dev = _dev()
    spec = _in(SP.spec_data(shape), dev)
    da, dph = (_in(t, dev) for t in SP.grad_data(shape))
    dspec = Out((B, 2, F, T), dev)
    _run("isi_spec_inverse_prepare_bwd_f32", _p(spec), _p(da), _p(dph), _p(dspec), B, T, F)
    _intact(spec, da, dph, dspec)
    SP.check_inverse_prepare_bwd(shape, dspec.view.cpu(), RECORD)


@pytest.mark.parametrize("case", SP.TILED_MEL_CASES, ids=SP.case_id)
def test_to_stft_and_its_adjoint(case):
    (B, T, F), mel = case
    dev = _dev()
    a, ph, dx = (_in(t, dev) for t in SP.to_stft_data(case))
    x = Out((B, T, 2 * F), dev)
    _run("isi_spec_to_stft_f32", _p(a), _p(ph), _p(x), B * T, F, mel)
    _intact(a, ph, x)
    SP.check_to_stft(case, x.view.cpu(), RECORD)
    da, dph = Out((B, T, F), dev), Out((B, T, F), dev)
    _run("isi_spec_to_stft_bwd_f32", _p(a), _p(ph), _p(dx), _p(da), _p(dph), B * T, F, mel)
    _intact(a, ph, dx, da, dph)
    SP.check_to_stft_bwd(case, da.view.cpu(), dph.view.cpu(), RECORD)


@pytest.mark.parametrize("case", SP.OLA_CASES, ids=SP.case_id)
def test_overlap_add(case):
    (n_fft, hop, left, T, L), B = case
    dev = _dev()
    for frames, t, k in SP.ola_impulses(case):
        fr, audio = _in(frames, dev), Out((B, L), dev)
        _run("isi_overlap_add_f32", _p(fr), _p(audio), B, T, n_fft, hop, left, L)
        _intact(fr, audio)
        SP.check_overlap_add_impulse(case, frames, t, k, audio.view.cpu())
    fr, audio = _in(SP.ola_noise(case), dev), Out((B, L), dev)
    _run("isi_overlap_add_f32", _p(fr), _p(audio), B, T, n_fft, hop, left, L)
    _intact(fr, audio)
    SP.check_overlap_add_noise(case, audio.view.cpu(), RECORD)


@pytest.mark.parametrize("case", SP.DIST_CASES, ids=SP.case_id)
def test_distance_sums(case):
    B, T, F, RS, rpb = case
    dev = _dev()
    nchunk = -(-T // rpb)
    for data, check in ((SP.distance_pins(case)[:2], SP.check_distance_pins), (SP.distance_noise(B, T, F, RS), SP.check_distance_noise)):
        xp, xt = (_in(t, dev) for t in data)
        partial = Out((B, nchunk, 4), dev)                            # exactly B ceil(T / rows_per_block) 4 values
        _run("isi_spec_distance_fwd_f32", _p(xp), _p(xt), _p(partial), B, T, F, RS, C.c_float(SP.DIST_EPS), rpb)
        _intact(xp, xt, partial)
        check(case, partial.view.cpu(), RECORD)


@pytest.mark.parametrize("case", SP.DIST_GRAD_CASES, ids=SP.case_id)
def test_distance_grad(case):
    B, T, F, RS, kind = case
    dev = _dev()
    xp, xt, clin, clog = (_in(t, dev) for t in SP.distance_grad_data(case))
    dx = Out((B, T, RS), dev)
    _run("isi_spec_distance_bwd_f32", _p(xp), _p(xt), _p(dx), _p(clin), _p(clog), B, T, F, RS, C.c_float(SP.DIST_EPS), kind)
    _intact(xp, xt, clin, clog, dx)
    SP.check_distance_grad(case, dx.view.cpu(), RECORD)


@pytest.mark.parametrize("case", SP.AFFINE_CASES, ids=SP.case_id)
def test_affine_mask(case):
    B, HW, with_ref, use_mask = case
    dev = _dev()
    x, ref = SP.affine_data(case)
    xd, rd = _in(x, dev), (_in(ref, dev) if ref is not None else None)
    y = Out((B, 2, HW), dev)
    coeffs = [C.c_float(v) for v in (*SP.AFFINE_COEFFS, SP.AFFINE_THR)]
    _run("isi_spec_affine_mask_f32", _p(xd), _p(rd) if rd is not None else None, _p(y), B, HW, *coeffs, use_mask)
    _intact(xd, y, *([rd] if rd is not None else []))
    SP.check_affine_mask(case, y.view.cpu(), RECORD)


# ------------------------------------------------------------------- the surfaces at F = 36, not a multiple of the 32-wide tile
@pytest.mark.parametrize("T", [1, 33])
@pytest.mark.parametrize("mel", [False, True])
def test_surfaces_at_36_bins(mel, T):
    """SpectrogramsHelper / MelSpectrogramsHelper at n_fft = 72, hop = 24 (F = 36): to_spectrogram, to_audio and the to_audio
    gradient against oracle/spectrogram_oracle.py under the tolerances of tests/test_spectrogram_gpu.py."""
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper, SpectrogramsHelper
    from oracle import spectrogram_oracle as S
    from test_spectrogram_gpu import _audio, _circ
    dev = _dev()
    n_fft, hop, B = 72, 24, 2
    cfg = S.SpecConfig(fs_hz=16000, n_fft=n_fft, hop_length=hop, window_length=n_fft)
    h = (MelSpectrogramsHelper if mel else SpectrogramsHelper)(16000, n_fft, hop, n_fft).to(dev)
    x = _audio(B, T * hop - 5, 100 + T)
    ref = S.to_spectrogram(cfg, x.double(), mel).float()
    got = h.to_spectrogram(x.to(dev)).cpu()
    assert got.shape == ref.shape == (B, 2, 36, T)
    if mel:
        assert torch.equal(torch.isfinite(got[:, 0]), torch.isfinite(ref[:, 0]))
    assert float((got[:, 0] - ref[:, 0]).abs().max()) <= 1e-3 * float(ref[:, 0].abs().max())
    if T > 1:
        bad = (_circ(got[:, 1, :, 1:], ref[:, 1, :, 1:]) > 2e-3).float().mean()
        assert float(bad) <= 1e-4, f"{float(bad):.2e} of the instantaneous frequencies differ"
    d0 = _circ(got[:, 1, :, 0], ref[:, 1, :, 0]) if not mel else (got[:, 1, :, 0] - ref[:, 1, :, 0]).abs()
    assert float((d0 > 2e-3).float().mean()) <= 1e-3
    # to_audio and its gradient, at the specification's own spectrogram
    w = torch.randn(B, T * hop, generator=torch.Generator().manual_seed(T))
    sd = ref.to(dev).requires_grad_(True)
    out = h.to_audio(sd)
    (out * w.to(dev)).sum().backward()
    sr = ref.double().requires_grad_(True)
    want = S.to_audio(cfg, sr, mel)
    (want * w.double()).sum().backward()
    assert out.shape == want.shape == (B, T * hop)
    assert float((out.detach().cpu() - want.detach().float()).abs().max()) <= 1e-3 * float(want.detach().abs().max())
    gr = sr.grad.float()
    for ch in (0, 1):
        err = (sd.grad[:, ch].cpu() - gr[:, ch]).abs().max() / gr[:, ch].abs().max()
        assert err <= 5e-3, f"channel {ch}: gradient error {err:.3e}"
