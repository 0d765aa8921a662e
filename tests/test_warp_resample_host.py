"""Host-side checks of the time-warped read (csrc/warp_resample.hip, isi_warp_resample_f32): its float64 specification
(tests/warp_resample_spec.py) is the polyphase resampler's at a constant rate and reads a tone along a curved map as
the ideal tone; the fp32 emulation of the kernel's weights stays inside the constant the bound is built from; the
comparison the GPU test uses accepts that emulation and rejects six planted faults; the library refuses bad arguments
before any launch.  No GPU needed."""
import math
import pathlib

import numpy as np
import pytest

import resample_spec as RS
import warp_resample_spec as S

FAKE = 0x10000      # non-null, 16-byte aligned, never dereferenced on the host


@pytest.mark.parametrize("num,den", [(3, 2), (2, 3), (160, 147), (4, 5)])
def test_spec_at_a_constant_rate_is_the_polyphase_resampler(num, den):
    """Reading at num / den samples per output, under the cutoff in float64, = `resample(x, num, den)`, whose table is
    rounded to fp32: within 2e-7 on unit-variance noise (the cutoff rounded to fp32 as well, as the kernel is given it,
    costs up to 4e-7 more: an fp32 cut is off by up to 6e-8 of itself, and so is every tap's t)."""
    g = np.random.default_rng(num * 1000 + den)
    x = g.standard_normal((1, 700)).astype(np.float32)
    pos, cut = S.constant_rate_rows(700, num, den)
    want = RS.resample(x, num, den)
    got = S.warp(x, pos[None], cut[None])
    assert got.y.shape == want.shape
    err = float(np.abs(got.y - want).max())
    print(f"rate {num}/{den}: max difference {err:.2e}")
    assert err <= 2e-7
    assert not got.zero.any()


@pytest.mark.parametrize("curve", ["vibrato", "glide"])
def test_spec_reads_a_tone_along_a_curved_map(curve):
    """A 3 kHz tone at 16 kHz read along the +-50 cent 6 Hz vibrato map, and along a glide up to rate 2, is the tone at the
    warped time within 1e-7 (measured 1.9e-8) away from the ends."""
    fs, L = 16000.0, 6000
    n = np.arange(L, dtype=np.float64)
    if curve == "vibrato":
        rate = 2.0 ** (0.5 / 12.0 * np.sin(2.0 * math.pi * 6.0 * n / fs))
        rate = rate[:4000]
    else:
        rate = np.linspace(1.0, 2.0, 3000)
    pos = np.cumsum(rate) - rate + 200.0
    assert pos[-1] < L - 200
    cut = (S.ROLLOFF * np.minimum(1.0, 1.0 / rate)).astype(np.float32)
    x = np.sin(2.0 * math.pi * 3000.0 * n / fs).astype(np.float32)[None]
    got = S.warp(x, pos[None], cut[None]).y[0]
    ideal = np.sin(2.0 * math.pi * 3000.0 * pos / fs)
    err = float(np.abs(got - ideal).max())
    print(f"{curve}: max difference {err:.2e}")
    assert err <= 1e-7


def test_emulated_weight_error_is_inside_the_constant():
    worst = S.measure_weight_error() * S.U
    print(f"largest |w32 - w64| / c = {worst / S.U:.3f} x 2^-24, E_W = {S.E_W / S.U:.3f} x 2^-24")
    assert worst <= S.E_W / 2.0
    assert S.E_W <= 2.0 * 1.01 * worst + 1e-12          # and the constant is that measurement, not a looser one


def test_cut_clamp_and_constants():
    c = S.clamp_cut(np.array([0.0, -1.0, 5.0, np.nan, 0.5, 0.2, 1.0, np.inf, -np.inf], dtype=np.float32))
    assert c.tolist() == [S.CUT_MIN, S.CUT_MIN, 1.0, S.CUT_MIN, 0.5, S.CUT_MIN, 1.0, 1.0, S.CUT_MIN]
    assert (S.Z, S.ROLLOFF, S.BETA) == (64, 0.9475937167399596, 14.769656459379492)
    assert 2 * int(S.Z / 0.2) + 1 == 641 and S.K_MAX == 321
    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "isi_hip.h").read_text()
    assert "#define ISI_WARP_CUT_MIN 0.2f" in header
    # the window polynomial: positive coefficients that sum to the window at t = 0
    assert (S.WIN_COEF > 0).all() and abs(float(S.WIN_COEF.astype(np.float64).sum()) - 1.0) < 1e-7


def _mutant_case():
    """60 100 samples of noise on a pedestal; fractional positions around sample 60 000 and across the far end; cuts
    inside and outside the clamp."""
    g = np.random.default_rng(7)
    L, N = 60100, 240
    x = (1.0 + g.standard_normal((2, L))).astype(np.float32)
    pos = np.concatenate([g.uniform(59900.0, 60040.0, N // 2), np.linspace(L - 30.0, L + 420.0, N // 2) + 0.37])
    cut = np.resize(np.array([0.5, 0.0, 5.0, S.ROLLOFF, 0.3, np.nan, 0.75], dtype=np.float32), N)
    return x, pos[None], cut[None]


def test_comparison_accepts_the_emulation_and_rejects_every_mutant():
    x, pos, cut = _mutant_case()
    spec = S.warp(x, pos, cut)
    ratio = S.compare(S.warp32(x, pos, cut), spec, "emulation")
    print(f"emulation: worst error / bound {ratio:.3f}")
    assert 0.0 < ratio <= 1.0
    assert spec.zero.any() and not spec.zero.all()
    for mutant in S.MUTANTS:
        wrong = S.warp(x, pos, cut, mutant=mutant).y.astype(np.float32)
        with pytest.raises(AssertionError):
            S.compare(wrong, spec, mutant)
    # -0.0 where +0.0 belongs, and a NaN, are not let through either
    bad = S.warp32(x, pos, cut)
    bad[spec.zero] = -0.0
    with pytest.raises(AssertionError, match="not \\+0.0"):
        S.compare(bad, spec)
    bad = S.warp32(x, pos, cut)
    bad[0, 0] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        S.compare(bad, spec)


def test_emulation_meets_the_bound_on_kernel_cases():
    worst = 0.0
    for case in (S.make_case(65, 300, 3, 3), S.make_case(1000, 65, 3, 3, seed=1), S.make_case(1, 63, 1, 1), S.make_case(2, 64, 3, 1)):
        worst = max(worst, S.compare(S.warp32(case.x, case.pos, case.cut), case.spec, case.name))
    print(f"emulation on four kernel cases: worst error / bound {worst:.3f}")
    kinds = set()
    for L in S.KERNEL_L:
        for N in S.KERNEL_N:
            for B in S.KERNEL_B:
                for pb in sorted({1, B}):
                    for seed in (0, 1):
                        first = (L + 3 * N + 5 * B + pb + seed) % S.N_ROW_KINDS
                        kinds |= {(first + 3 * r) % S.N_ROW_KINDS for r in range(pb)}
    assert kinds == set(range(S.N_ROW_KINDS))           # every kind of row is walked by the GPU test


def test_argument_checks_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    ok = dict(x=FAKE, xs=1000, pos=FAKE, cut=FAKE, pb=1, y=FAKE, ys=300, B=2, L=1000, N=300)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.isi_warp_resample_f32(a["x"], a["xs"], a["pos"], a["cut"], a["pb"], a["y"], a["ys"], a["B"], a["L"], a["N"],
                                         None)
    for name in ("x", "pos", "cut", "y"):
        assert call(**{name: None}) == -1 and b"null" in lib.isi_last_error()
    for name in ("x", "cut", "y"):
        assert call(**{name: FAKE + 2}) == -1 and b"aligned" in lib.isi_last_error()
    assert call(pos=FAKE + 4) == -1 and b"double" in lib.isi_last_error()
    assert call(B=0) == -1 and call(L=0) == -1 and call(N=0) == -1 and call(B=-3) == -1
    assert call(pb=0) == -1 and call(pb=3) == -1 and b"pos_batch" in lib.isi_last_error()
    assert call(xs=999) == -1 and b"stride" in lib.isi_last_error()
    assert call(ys=299) == -1 and b"stride" in lib.isi_last_error()
    assert call(L=1 << 31, xs=1 << 31) == -4 and b"2^31" in lib.isi_last_error()
    assert call(N=1 << 31, ys=1 << 31) == -4 and b"2^31" in lib.isi_last_error()
