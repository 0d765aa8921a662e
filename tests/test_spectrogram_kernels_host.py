"""What tests/test_spectrogram_kernels_gpu.py measures the kernels of csrc/spectrogram.hip with, checked without a GPU: the
float64 specifications of tests/spectrogram_spec.py against independent formulations (oracle/spectrogram_oracle.py, float64
torch.cumsum, float64 autograd), mutants of the float32 yardsticks -- each imitates a way a kernel could be wrong and must be
rejected by the very rule the GPU file applies to that kernel --, the unmutated yardsticks under every rule of every GPU case,
and the refusals of the C-ABI that happen on the host."""
import math

import pytest
import torch

import spectrogram_spec as SP
import tests_support as TS
from oracle import spectrogram_oracle as O

F64 = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------- specs against independent formulations, 1e-12
def test_wrap_is_the_oracles():
    g = _g(1)
    d = torch.cat([torch.randn(5000, generator=g, dtype=F64) * 30.0, torch.tensor([0.0, math.pi, -math.pi, 3 * math.pi, -3 * math.pi,
                                                                                      2 * math.pi, -2 * math.pi], dtype=F64)])
    assert float((SP.wrap(d) - O.wrap(d)).abs().max()) <= 1e-12
    assert SP.wrap(torch.tensor([math.pi, -math.pi], dtype=F64)).tolist() == [math.pi, -math.pi]
    assert SP.wrap_margin(torch.tensor([3 * math.pi + 0.25, 0.0])) == pytest.approx(0.25)


@pytest.mark.parametrize("mel", [0, 1])
def test_polar_and_finish_equal_the_oracle(mel):
    B, T, F = 2, 70, 9
    g = _g(2 + mel)
    X = torch.complex(torch.randn(B, F, T, generator=g, dtype=F64), torch.randn(B, F, T, generator=g, dtype=F64)).to(torch.complex64)
    stft = torch.cat([X.real.transpose(1, 2), X.imag.transpose(1, 2)], -1).contiguous()       # [B,T,2F] float32
    mag, ang = X.to(torch.complex128).abs(), torch.angle(X.to(torch.complex128))              # the oracle's [B,F,T]
    a, ph = SP.polar(stft, mel)
    assert a.dtype == F64 and a.shape == (B, T, F)
    if mel:
        want_a, want_ph = mag * mag, O.unwrap(ang)
    else:
        want_a, want_ph = torch.log(mag + O.EPS), ang
    assert TS.row_error(a, want_a.transpose(1, 2)) <= 1e-12 and TS.row_error(ph, want_ph.transpose(1, 2)) <= 1e-12
    # finish on the float32 intermediates a kernel would be handed
    a32, ph32 = a.float(), (ph * (7.0 if mel else 1.0)).float()
    out = SP.finish(a32, ph32, mel)
    want0 = torch.log(a32.double() + O.EPS) if mel else a32.double()
    want = torch.stack([want0.transpose(1, 2), O.instantaneous_frequency(ph32.double().transpose(1, 2))], 1)
    assert out.shape == (B, 2, F, T) and TS.row_error(out, want) <= 1e-12
    assert TS.row_error(SP.finish(a32[:, :1], ph32[:, :1], mel), want[..., :1]) <= 1e-12       # T == 1


def test_inverse_prepare_equals_cumsum_and_to_stft_equals_polar():
    B, T, F = 2, 77, 5
    g = _g(4)
    spec = torch.stack([torch.randn(B, F, T, generator=g), torch.rand(B, F, T, generator=g) * 2 - 1], 1)
    a, ph = SP.inverse_prepare(spec)
    want_ph = torch.cumsum(spec[:, 1].double() * math.pi, -1).transpose(1, 2)
    assert TS.row_error(a, torch.exp(spec[:, 0].double()).transpose(1, 2)) <= 1e-12 and TS.row_error(ph, want_ph) <= 1e-12
    bound = SP.inverse_prepare_bound(spec)
    assert bound.shape == ph.shape and bool((bound[:, 1:] >= bound[:, :-1]).all())
    for mel in (0, 1):
        a32 = (torch.randn(B, T, F, generator=g) * 2).float() if mel else a.float()
        ph32 = ph.float()
        mag = torch.exp(0.5 * torch.log(a32.double().clamp_min(0) + O.EPS)) if mel else a32.double()     # the oracle's to_audio
        X = torch.polar(mag, ph32.double())
        assert TS.row_error(SP.to_stft(a32, ph32, mel), torch.cat([X.real, X.imag], -1)) <= 1e-12


@pytest.mark.parametrize("geom", [(16, 4, 12, 5, 20), (256, 50, 0, 7, 556), (64, 24, 0, 3, 112), (16, 4, 0, 3, 40), (16, 4, 12, 1, 4)])
def test_overlap_add_equals_the_oracles_loop(geom):
    n_fft, hop, left, T, L = geom
    frames = torch.randn(2, T, n_fft, generator=_g(5))
    total = max((T - 1) * hop + n_fft, left + L)
    out = torch.zeros(2, total, dtype=F64)
    for t in range(T):                                               # oracle/spectrogram_oracle.py::to_audio
        out[:, t * hop:t * hop + n_fft] += frames[:, t].double()
    got, bound = SP.overlap_add(frames, hop, left, L, with_bound=True)
    assert got.shape == (2, L) and TS.row_error(got, out[:, left:left + L]) <= 1e-12
    assert bool(((bound == 0) == (got == 0)).all())


@pytest.mark.parametrize("mel", [0, 1])
def test_to_stft_bwd_equals_autograd(mel):
    g = _g(6 + mel)
    a = (torch.rand(3, 11, 7, generator=g) + 0.1).float()            # away from a <= 0
    ph = (torch.randn(3, 11, 7, generator=g) * 5).float()
    dx = torch.randn(3, 11, 14, generator=g)
    ad, pd = a.double().requires_grad_(True), ph.double().requires_grad_(True)
    mag = torch.sqrt(ad.clamp_min(0) + SP.EPS) if mel else ad
    (torch.cat([mag * torch.cos(pd), mag * torch.sin(pd)], -1) * dx.double()).sum().backward()
    da, dph = SP.to_stft_bwd(a, ph, dx, mel)
    assert TS.row_error(da, ad.grad) <= 1e-12 and TS.row_error(dph, pd.grad) <= 1e-12
    if mel:                                                          # the documented choice at and below the kink
        a[0, 0, :3] = torch.tensor([0.0, -1.0, -1e-9])
        assert SP.to_stft_bwd(a, ph, dx, 1)[0][0, 0, :3].tolist() == [0.0, 0.0, 0.0]


def test_inverse_prepare_bwd_equals_autograd():
    B, T, F = 2, 70, 5
    g = _g(8)
    spec = torch.stack([torch.randn(B, F, T, generator=g), torch.rand(B, F, T, generator=g) * 2 - 1], 1)
    da, dph = torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)
    s = spec.double().requires_grad_(True)
    a = torch.exp(s[:, 0]).transpose(1, 2)
    ph = torch.cumsum(s[:, 1] * math.pi, -1).transpose(1, 2)
    ((a * da.double()).sum() + (ph * dph.double()).sum()).backward()
    assert TS.row_error(SP.inverse_prepare_bwd(spec, da, dph), s.grad) <= 1e-12
    assert SP.inverse_prepare_bwd_bound(dph).shape == (B, F, T)


@pytest.mark.parametrize("kind", [0, 1])
def test_distance_specs_equal_autograd(kind):
    B, T, F, RS, eps = 2, 5, 9, 24, 2.0 ** -10
    g = _g(9 + kind)
    xp, xt = torch.randn(B, T, RS, generator=g), torch.randn(B, T, RS, generator=g) * 1.5        # away from |Xp| = 0 and dm = 0
    clin, clog = torch.rand(B, generator=g) + 0.5, torch.rand(B, generator=g) + 0.5
    p = xp.double().requires_grad_(True)
    mp = torch.sqrt(p[..., :F] ** 2 + p[..., F:2 * F] ** 2)
    mt = torch.sqrt(xt.double()[..., :F] ** 2 + xt.double()[..., F:2 * F] ** 2)
    dm, dl = mp - mt, torch.log(mp + eps) - torch.log(mt + eps)
    assert float(dm.detach().abs().min()) > 1e-6
    gfun = (lambda v: v.abs()) if kind == 0 else (lambda v: 0.5 * v * v)
    loss = (clin.double().view(-1, 1, 1) * gfun(dm) + clog.double().view(-1, 1, 1) * gfun(dl)).sum()
    loss.backward()
    got = SP.distance_grad(xp, xt, clin, clog, F, RS, eps, kind)
    assert TS.row_error(got, p.grad) <= 1e-12 and bool((got[..., 2 * F:] == 0).all())
    # the sums, chunk by chunk, against the same terms summed by slicing
    for rpb in (1, 2, 5, 9):
        sums = SP.distance_sums(xp, xt, F, RS, eps, rpb)
        assert sums.shape == (B, -(-T // rpb), 4)
        for c in range(sums.shape[1]):
            sl = slice(c * rpb, min(T, (c + 1) * rpb))
            want = torch.stack([v[:, sl].detach().sum((1, 2)) for v in (dm.abs(), dm * dm, dl.abs(), dl * dl)], -1)
            assert TS.row_error(sums[:, c], want) <= 1e-12
    # |Xp| = 0: gradient 0; sign(0) = 0
    xp[0, 0, 0], xp[0, 0, F] = 0.0, 0.0
    xt[1, 1, 2], xt[1, 1, F + 2] = xp[1, 1, 2], xp[1, 1, F + 2]
    got = SP.distance_grad(xp, xt, clin, clog, F, RS, eps, kind)
    assert got[0, 0, 0] == 0 and got[0, 0, F] == 0 and bool(torch.isfinite(got).all())
    assert got[1, 1, 2] == 0 and got[1, 1, F + 2] == 0


def test_affine_mask_equals_the_oracle():
    g = _g(11)
    x = torch.stack([torch.randn(2, 40, generator=g) * 3 - 3, torch.rand(2, 40, generator=g)], 1)
    a0, b0, a1, b1 = SP.AFFINE_COEFFS
    x4 = x.double().view(2, 2, 5, 8)
    aff = x4 * torch.tensor([a0, a1], dtype=F64).view(1, 2, 1, 1) + torch.tensor([b0, b1], dtype=F64).view(1, 2, 1, 1)
    want = O.mask_phase(aff, SP.AFFINE_THR).view(2, 2, 40)
    assert TS.row_error(SP.affine_mask(x, None, a0, b0, a1, b1, SP.AFFINE_THR, 1), want) <= 1e-12
    assert TS.row_error(SP.affine_mask(x, None, a0, b0, a1, b1, SP.AFFINE_THR, 0), aff.view(2, 2, 40)) <= 1e-12
    ref = torch.randn(2, 2, 40, generator=g) * 2 - 2
    ref[:, 0, ::3] = SP.AFFINE_THR
    want = torch.where((ref[:, 0].double() <= SP.AFFINE_THR), torch.zeros(2, 40, dtype=F64), aff.view(2, 2, 40)[:, 1])
    assert TS.row_error(SP.affine_mask(x, ref, a0, b0, a1, b1, SP.AFFINE_THR, 1)[:, 1], want) <= 1e-12


# ------------------------------------------------------------------------------ the unmutated yardsticks pass every rule
@pytest.mark.parametrize("case", SP.POLAR_CASES, ids=SP.case_id)
def test_yardstick_polar(case):
    SP.check_polar(case, *SP.polar_f32(SP.polar_data(case), case[1]))


@pytest.mark.parametrize("case", SP.TILED_MEL_CASES, ids=SP.case_id)
def test_yardstick_finish_to_stft_and_adjoint(case):
    a, ph = SP.finish_data(case)
    SP.check_finish(case, SP.finish_f32(a, ph, case[1]))
    a, ph, dx = SP.to_stft_data(case)
    SP.check_to_stft(case, SP.to_stft_f32(a, ph, case[1]))
    SP.check_to_stft_bwd(case, *SP.to_stft_bwd_f32(a, ph, dx, case[1]))


def test_mel_phases_reach_a_few_hundred():
    _, ph = SP.finish_data(((3, 100, 33), 1))
    assert float(ph.abs().max()) > 200.0
    _, ph, _ = SP.to_stft_data(((3, 100, 33), 1))
    assert float(ph.abs().max()) > 200.0


def test_yardstick_finish_wrap_ends():
    a, ph, steps = SP.wrap_end_data()
    P = float(torch.tensor(math.pi, dtype=torch.float32))
    assert steps.tolist() == [P, -P, float(torch.tensor(3 * P, dtype=torch.float32)), -float(torch.tensor(3 * P, dtype=torch.float32)),
                              2 * P, -2 * P, 0.0]
    SP.check_finish_wrap_ends(SP.finish_f32(a, ph, 0))


@pytest.mark.parametrize("shape", SP.SCAN_CASES, ids=SP.case_id)
def test_yardstick_scans(shape):
    """The sequential float32 scans stay inside the derived bound at every T up to 1000."""
    rec = []
    SP.check_inverse_prepare(shape, *SP.inverse_prepare_f32(SP.spec_data(shape)), record=rec)
    SP.check_inverse_prepare_bwd(shape, SP.inverse_prepare_bwd_f32(SP.spec_data(shape), *SP.grad_data(shape)), record=rec)
    assert all(c.ratio <= 0.6 for c in rec if "running sum" in c.what), [c for c in rec if "running sum" in c.what]


@pytest.mark.parametrize("case", SP.OLA_CASES, ids=SP.case_id)
def test_yardstick_overlap_add(case):
    (n_fft, hop, left, T, L), B = case
    SP.check_overlap_add_noise(case, SP.overlap_add(SP.ola_noise(case), hop, left, L, dtype=torch.float32))
    for fr, t, k in SP.ola_impulses(case):
        SP.check_overlap_add_impulse(case, fr, t, k, SP.overlap_add(fr, hop, left, L, dtype=torch.float32))
    if (n_fft, hop, left, T, L) == (16, 4, 0, 3, 40):                # L past the last frame: the tail is untouched
        assert bool((SP.overlap_add(SP.ola_noise(case), hop, left, L)[:, 24:] == 0).all())


@pytest.mark.parametrize("case", SP.DIST_CASES, ids=SP.case_id)
def test_yardstick_distance_sums(case):
    B, T, F, RS, rpb = case
    xp, xt = SP.distance_noise(B, T, F, RS)
    assert RS == 2 * F or bool(torch.isnan(xp[..., 2 * F:]).all())
    SP.check_distance_noise(case, SP.distance_sums(xp, xt, F, RS, SP.DIST_EPS, rpb, dtype=torch.float32))
    xp, xt, owners = SP.distance_pins(case)
    SP.check_distance_pins(case, SP.distance_sums(xp, xt, F, RS, SP.DIST_EPS, rpb, dtype=torch.float32))
    # a dropped element is rejected at these sizes
    xp, xt = SP.distance_noise(B, T, F, RS)
    with pytest.raises(AssertionError):
        SP.check_distance_noise(case, SP.distance_sums(xp, xt, F, RS, SP.DIST_EPS, rpb, dtype=torch.float32, drop_last=True))


def test_distance_cases_cover_what_the_issue_names():
    assert {c[2] for c in SP.DIST_CASES} == {33, 129, 1025} and {c[1] for c in SP.DIST_CASES} == {1, 7, 20}
    assert {c[0] for c in SP.DIST_CASES} == {1, 3}
    for F in (33, 129, 1025):
        assert {c[3] for c in SP.DIST_CASES if c[2] == F} == {2 * F, (2 * F + 3) // 4 * 4, 2 * F + 8}
    assert all(min(c[4], c[1]) * c[2] <= 1100 for c in SP.DIST_CASES)
    assert any(c[1] % c[4] and c[4] < c[1] and c[0] == 3 for c in SP.DIST_CASES)                  # a ragged last chunk, B = 3
    assert any(c[4] > c[1] for c in SP.DIST_CASES)


@pytest.mark.parametrize("case", SP.DIST_GRAD_CASES, ids=SP.case_id)
def test_yardstick_distance_grad(case):
    B, T, F, RS, kind = case
    xp, xt, clin, clog = SP.distance_grad_data(case)
    SP.check_distance_grad(case, SP.distance_grad(xp, xt, clin, clog, F, RS, SP.DIST_EPS, kind, dtype=torch.float32))


@pytest.mark.parametrize("case", SP.AFFINE_CASES, ids=SP.case_id)
def test_yardstick_affine_mask(case):
    x, ref = SP.affine_data(case)
    SP.check_affine_mask(case, SP.affine_mask(x, ref, *SP.AFFINE_COEFFS, SP.AFFINE_THR, case[3], dtype=torch.float32))


def test_affine_cases_cover_what_the_issue_names():
    assert {c[1] // 4 for c in SP.AFFINE_CASES} == {1, 255, 257} and {c[0] for c in SP.AFFINE_CASES} == {1, 3}
    assert {(c[2], c[3]) for c in SP.AFFINE_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---------------------------------------------------------------------------------------------------------- the mutants
def _rejects(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_mutant_scan_carry_dropped_at_frame_32():
    for shape in ((1, 33, 33), (3, 65, 36), SP.SCAN_LONG):
        spec, (da, dph) = SP.spec_data(shape), SP.grad_data(shape)
        rec = []
        _rejects(SP.check_inverse_prepare, shape, *SP.inverse_prepare_f32(spec, drop_carry_at=32), record=rec)
        _rejects(SP.check_inverse_prepare_bwd, shape, SP.inverse_prepare_bwd_f32(spec, da, dph, drop_carry_at=32), record=rec)
        assert len(rec) == 4 and all(c.ratio > 100 for c in rec if "running sum" in c.what), rec


def test_mutant_scan_carry_shared_between_neighbouring_frequencies():
    for shape in ((1, 33, 33), (3, 65, 36)):
        spec, (da, dph) = SP.spec_data(shape), SP.grad_data(shape)
        _rejects(SP.check_inverse_prepare, shape, *SP.inverse_prepare_f32(spec, share_carry=True))
        _rejects(SP.check_inverse_prepare_bwd, shape, SP.inverse_prepare_bwd_f32(spec, da, dph, share_carry=True))


def test_mutant_wrap_without_the_end_convention():
    a, ph, _ = SP.wrap_end_data()
    _rejects(SP.check_finish_wrap_ends, SP.finish_f32(a, ph, 0, end_convention=False))


def test_mutant_first_frame_differenced():
    for case in (((1, 33, 33), 1), ((3, 1, 31), 1)):
        a, ph = SP.finish_data(case)
        _rejects(SP.check_finish, case, SP.finish_f32(a, ph, 1, first_differenced=True))


def test_mutant_finish_differences_forward():
    for case in (((1, 2, 33), 0), ((1, 33, 33), 1)):
        a, ph = SP.finish_data(case)
        _rejects(SP.check_finish, case, SP.finish_f32(a, ph, case[1], forward_difference=True))


@pytest.mark.parametrize("mutant", [dict(t_hi_off=-1), dict(break_past=True), dict(ignore_left=True)], ids=lambda m: next(iter(m)))
def test_mutant_overlap_add_window(mutant):
    """The noise rule rejects each window mutant at every geometry it changes; the impulse rule rejects it on at least one
    impulse of such a geometry."""
    changed = 0
    for case in SP.OLA_CASES:
        (n_fft, hop, left, T, L), B = case
        bad = SP.overlap_add(SP.ola_noise(case), hop, left, L, dtype=torch.float32, **mutant)
        good = SP.overlap_add(SP.ola_noise(case), hop, left, L, dtype=torch.float32)
        if SP.same_bits(bad, good):                                   # (left = 0, or one frame whose every k >= hop)
            continue
        changed += 1
        _rejects(SP.check_overlap_add_noise, case, bad)
        hits = 0
        for fr, t, k in SP.ola_impulses(case):
            try:
                SP.check_overlap_add_impulse(case, fr, t, k, SP.overlap_add(fr, hop, left, L, dtype=torch.float32, **mutant))
            except AssertionError:
                hits += 1
        assert hits >= 1, (case, mutant)
    assert changed >= 6


def test_mutant_distance_chunk_edge_unclamped():
    hit = 0
    for case in SP.DIST_CASES:
        B, T, F, RS, rpb = case
        if B == 1 or T % rpb == 0:
            continue
        hit += 1
        xp, xt = SP.distance_noise(B, T, F, RS)
        _rejects(SP.check_distance_noise, case, SP.distance_sums(xp, xt, F, RS, SP.DIST_EPS, rpb, dtype=torch.float32, unclamped=True))
    assert hit >= 3
    # the pins: the last chunk of sample 0 would count the first rows of sample 1
    case = next(c for c in SP.DIST_CASES if c[0] == 3 and c[4] > c[1] > 1)
    B, T, F, RS, rpb = case
    xp, xt, _ = SP.distance_pins(case)
    _rejects(SP.check_distance_pins, case, SP.distance_sums(xp, xt, F, RS, SP.DIST_EPS, rpb, dtype=torch.float32, unclamped=True))


def test_mutant_distance_imaginary_block_one_column_early():
    for case in SP.DIST_CASES[::5]:
        B, T, F, RS, rpb = case
        xp, xt = SP.distance_noise(B, T, F, RS)
        _rejects(SP.check_distance_noise, case, SP.distance_sums(xp, xt, F, RS, SP.DIST_EPS, rpb, dtype=torch.float32, im_off=1))
        xp, xt, _ = SP.distance_pins(case)
        _rejects(SP.check_distance_pins, case, SP.distance_sums(xp, xt, F, RS, SP.DIST_EPS, rpb, dtype=torch.float32, im_off=1))


def test_mutant_distance_grad_padding_unwritten():
    hit = 0
    for case in SP.DIST_GRAD_CASES:
        B, T, F, RS, kind = case
        if RS == 2 * F:
            continue
        hit += 1
        xp, xt, clin, clog = SP.distance_grad_data(case)
        _rejects(SP.check_distance_grad, case,
                 SP.distance_grad(xp, xt, clin, clog, F, RS, SP.DIST_EPS, kind, dtype=torch.float32, write_padding=False))
    assert hit >= 6


def test_mutant_mask_strictly_below_the_threshold():
    hit = 0
    for case in SP.AFFINE_CASES:
        if not (case[2] and case[3]):
            continue
        hit += 1
        x, ref = SP.affine_data(case)
        _rejects(SP.check_affine_mask, case, SP.affine_mask(x, ref, *SP.AFFINE_COEFFS, SP.AFFINE_THR, 1, dtype=torch.float32, strict=True))
    assert hit == 3


def test_mutant_mel_magnitude_without_the_clamp():
    for case in (((1, 1, 33), 1), ((3, 65, 36), 1)):
        a, ph, _ = SP.to_stft_data(case)
        assert bool((a < -SP.EPS).any()) and bool((a == 0).any())
        _rejects(SP.check_to_stft, case, SP.to_stft_f32(a, ph, 1, clamp=False))


# ------------------------------------------------------------------------------------------------ refusals on the host
FAKE = 0x10000       # non-null, 16-byte aligned, never dereferenced on the host
INVALID = -1


def _refused(L, name, good, bad_variants):
    """Every variant of the valid argument list `good` ({position: value}) must return the invalid-argument code."""
    fn = getattr(L, name)
    for change in bad_variants:
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert fn(*args, None) == INVALID, f"{name}{tuple(args)} was not refused"
        assert L.isi_last_error(), name


def test_spectrogram_refusals_need_no_gpu():
    """Every refusal is decided before any launch: the pointers are fake and no device is touched."""
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    nulls = lambda n: [{i: None} for i in range(n)]
    nonpos = lambda idx: [{i: v} for i in idx for v in (0, -1)]
    big_b = lambda i: [{i: 65536}]
    # (B, T, F, mel) kernels
    for name in ("isi_spec_polar_f32", "isi_spec_finish_f32"):
        _refused(L, name, [FAKE, FAKE, FAKE, 2, 5, 9, 0], nulls(3) + nonpos((3, 4, 5)) + big_b(3))
    _refused(L, "isi_spec_finish_f32", [FAKE, FAKE, FAKE, 2, 5, 9, 0], [{4: 65535 * 32 + 1}])        # more than 65535 frame tiles
    _refused(L, "isi_spec_inverse_prepare_f32", [FAKE, FAKE, FAKE, 2, 5, 9], nulls(3) + nonpos((3, 4, 5)) + big_b(3))
    _refused(L, "isi_spec_inverse_prepare_bwd_f32", [FAKE, FAKE, FAKE, FAKE, 2, 5, 9], nulls(4) + nonpos((4, 5, 6)) + big_b(4))
    _refused(L, "isi_spec_to_stft_f32", [FAKE, FAKE, FAKE, 10, 9, 1], nulls(3) + nonpos((3, 4)))
    _refused(L, "isi_spec_to_stft_bwd_f32", [FAKE, FAKE, FAKE, FAKE, FAKE, 10, 9, 1], nulls(5) + nonpos((5, 6)))
    # overlap-add: frames, audio, B, T, n_fft, hop, left, L
    _refused(L, "isi_overlap_add_f32", [FAKE, FAKE, 2, 5, 16, 4, 12, 20], nulls(2) + nonpos((2, 3, 4, 5, 7)) + big_b(2) + [{6: -1}])
    # distance: RS < 2F, rows_per_block, kind
    fwd = [FAKE, FAKE, FAKE, 2, 5, 9, 18, 1e-3, 3]
    _refused(L, "isi_spec_distance_fwd_f32", fwd, nulls(3) + nonpos((3, 4, 5, 8)) + big_b(3) + [{6: 17}, {6: 0}])
    bwd = [FAKE, FAKE, FAKE, FAKE, FAKE, 2, 5, 9, 18, 1e-3, 0]
    _refused(L, "isi_spec_distance_bwd_f32", bwd, nulls(5) + nonpos((5, 6, 7)) + big_b(5) + [{8: 17}, {10: 2}, {10: -1}])
    # affine: x, ref, y, B, HW, a0, b0, a1, b1, thr, use_mask; `ref` may be null
    aff = [FAKE, FAKE, FAKE, 2, 8, 1.0, 0.0, 1.0, 0.0, 0.0, 1]
    _refused(L, "isi_spec_affine_mask_f32", aff, [{0: None}, {2: None}] + nonpos((3, 4)) + big_b(3) +
             [{4: 6}, {4: 9}, {0: FAKE + 4}, {1: FAKE + 8}, {2: FAKE + 12}])
    assert b"multiple of 4" in L.isi_last_error()
