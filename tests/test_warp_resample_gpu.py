"""isi_warp_resample_f32 (csrc/warp_resample.hip) against its float64 specification (tests/warp_resample_spec.py, which also
holds the cases, the bound and the comparison).

Kernel cases: L in {1, 2, 65, 1000} x N_out in {1, 63, 64, 65, 300} x B in {1, 3} x both pos_batch forms, twice.  Rows of
positions: rate 1 on the integers, constant 3/2 and 2/3, vibrato, a glide down to the cut's clamp, decreasing, random,
straddling 0 and L out to where the support ends, +-1e12 / +-3e9 / 1e300 / infinite / NaN; cuts ROLLOFF min(1, 1 / rate)
and 0, negative, 5, NaN; data: normal noise, impulses at 0 and L - 1, all ones.  The output sits inside a poisoned buffer,
the inputs are checked unchanged, outputs without a source must be +0.0.  The bound: E_W c S1 + (N + 2) 2^-24 S2, derived in
the spec file -- nothing to tune.

Figures of an MI355X run (profiles/warp_resample_checks.txt holds every case): the worst of the 123 cases reaches 0.374 of its
bound (L = 1, N_out = 300, the cuts 0 / negative / 5 / NaN) -- the figure the spec's fp32 emulation shows on that case; the
rates 3/2 and 2/3 differ from isi_resample_f32's output by 6.0e-7 / 9.5e-7, 0.7 % / 1.1 % of the two bounds' sum.

A recording aid, not a check: with ISI_WARP_RECORD=<file> in the environment the worst error / bound ratio of every kernel
case is written there when the module ends."""
import os

import numpy as np
import pytest
import torch

import resample_spec as RS
import warp_resample_spec as S

pytestmark = pytest.mark.gpu

RECORD = []      # (ratio, case name)
GUARD = 64       # floats of poison in front of and behind an output buffer


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("ISI_WARP_RECORD")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("# worst error / bound of isi_warp_resample_f32 against the float64 spec, per case of tests/test_warp_resample_gpu.py;\n"
                "# the bound: tests/warp_resample_spec.py (E_W c S1 + (N + 2) 2^-24 S2).  Worst first; outputs without a source are\n"
                "# compared with +0.0 bit for bit in every case.\n")
        for ratio, what in sorted(RECORD, key=lambda r: -r[0]):
            f.write(f"{ratio:8.3f}  {what}\n")


def _run(x, pos, cut, x_pad=0, y_pad=0):
    """x float32 [B, L], pos float64 [pb, N], cut float32 [pb, N] (numpy) -> y [B, N] (numpy) through the library: the
    output inside a poisoned buffer, rows x_pad / y_pad floats further apart than they are long"""
    from interactive_spectrogram_inpainting import _hip
    lib, dev = _hip.lib(), _dev()
    B, L = x.shape
    pb, N = pos.shape
    xs, ys = L + x_pad, N + y_pad
    xw = np.full((B, xs), 1e30, dtype=np.float32)          # what lies between the rows must never be read into a sum
    xw[:, :L] = x
    xd = torch.from_numpy(xw).to(dev)
    pd, cd = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(cut, dtype=np.float32)).to(dev)
    n = B * ys
    buf = torch.full((GUARD + n + GUARD,), S.OUT_POISON, dtype=torch.int32, device=dev)
    out = buf[GUARD:GUARD + n].view(torch.float32)
    rc = lib.isi_warp_resample_f32(xd.data_ptr(), xs, pd.data_ptr(), cd.data_ptr(), pb, out.data_ptr(), ys, B, L, N,
                                   _hip.stream_ptr(dev))
    assert rc == 0, lib.isi_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == S.OUT_POISON).all() and (host[GUARD + n:] == S.OUT_POISON).all(), "a write outside the output"
    rows = host[GUARD:GUARD + n].reshape(B, ys)
    assert (rows[:, N:] == S.OUT_POISON).all(), "a write into the gap between two output rows"
    assert np.array_equal(S.bits(xd.cpu().numpy()), S.bits(xw)), "the kernel changed x"
    assert np.array_equal(pd.cpu().numpy().view(np.int64), np.ascontiguousarray(pos, dtype=np.float64).view(np.int64)), "the kernel changed pos"
    assert np.array_equal(S.bits(cd.cpu().numpy()), S.bits(cut)), "the kernel changed cut"
    return np.ascontiguousarray(rows[:, :N]).view(np.float32)


@pytest.mark.parametrize("L", S.KERNEL_L)
def test_kernel_against_the_spec(L):
    for N in S.KERNEL_N:
        for B in S.KERNEL_B:
            for pos_batch in sorted({1, B}):
                for seed in (0, 1):
                    case = S.make_case(L, N, B, pos_batch, seed)
                    got = _run(case.x, case.pos, case.cut)
                    ratio = S.compare(got, case.spec, case.name)
                    print(f"{case.name}: worst error / bound = {ratio:.3f}")
                    RECORD.append((ratio, case.name))


def test_wide_strides_and_the_gap_between_rows():
    """x_stride > L and y_stride > N_out: the samples between two rows of x (1e30 each) reach no sum, the floats between two
    rows of y keep their poison (`_run` checks it)"""
    case = S.make_case(65, 300, 3, 3, seed=2)
    got = _run(case.x, case.pos, case.cut, x_pad=7, y_pad=5)
    ratio = S.compare(got, case.spec, case.name)
    RECORD.append((ratio, case.name + " x_stride=L+7 y_stride=N+5"))
    assert np.array_equal(S.bits(got), S.bits(_run(case.x, case.pos, case.cut)))


def test_a_row_has_the_same_bits_alone_and_inside_a_batch():
    case = S.make_case(1000, 300, 3, 3, seed=3)
    full = _run(case.x, case.pos, case.cut)
    for b in range(3):
        alone = _run(case.x[b:b + 1], case.pos[b:b + 1], case.cut[b:b + 1])
        assert np.array_equal(S.bits(alone[0]), S.bits(full[b])), f"row {b}"
    shared = _run(case.x, case.pos[1:2], case.cut[1:2])                      # pos_batch = 1: every row along row 1's map
    assert np.array_equal(S.bits(shared[1]), S.bits(full[1]))
    assert np.array_equal(S.bits(shared[0]), S.bits(_run(case.x[0:1], case.pos[1:2], case.cut[1:2])[0]))


@pytest.mark.parametrize("num,den", [(3, 2), (2, 3)])
def test_constant_rate_against_the_polyphase_kernel(num, den):
    """Reading at the constant rate num / den is the conversion num -> den of isi_resample_f32: the two kernels' outputs differ
    by at most the sum of their bounds (each against its own float64 specification; the specifications themselves differ by
    the cut's rounding to fp32, which this sum has to cover too)."""
    from GANsynth_pytorch import resample as R
    dev = _dev()
    g = np.random.default_rng(num)
    x = g.standard_normal((3, 1000)).astype(np.float32)
    pos, cut = S.constant_rate_rows(1000, num, den)
    cut = cut.astype(np.float32)
    spec = S.warp(x, pos[None], cut[None])
    got = _run(x, pos[None], cut[None])
    RECORD.append((S.compare(got, spec), f"L=1000 B=3 constant rate {num}/{den}"))
    orig, new, width, taps = RS.geometry(num, den)
    table = torch.from_numpy(RS.table32(num, den).T.copy()).to(dev)
    poly = R._run(torch.from_numpy(x).to(dev), orig, new, width, table).cpu().numpy().astype(np.float64)
    _, scale = RS.resample(x, num, den, with_abs=True)
    assert poly.shape == got.shape
    both = spec.bound + (taps + 2) * 2.0 ** -24 * scale
    err = np.abs(got.astype(np.float64) - poly)
    print(f"rate {num}/{den}: largest difference between the two kernels {err.max():.3e}, largest difference / sum of bounds "
          f"{(err / both).max():.3f}")
    assert (err <= both).all()


def test_far_positions_touch_nothing():
    """|p| beyond 2^31, 2^63 and the floats' range, in every lane of several blocks: every output +0.0 (`_run` holds the
    guards)"""
    N = 700
    x = np.ones((2, 65), dtype=np.float32)
    pos = np.resize(np.array([2.0 ** 31, -2.0 ** 31, 2.0 ** 32 + 7.5, -2.0 ** 40, 2.0 ** 63, -2.0 ** 63, 1e19, -1e19, 1e300, -1e300,
                              np.inf, -np.inf, np.nan, 466.0, -401.5]), N)[None]
    cut = np.resize(np.array([1.0, 0.2, np.nan, 0.0], dtype=np.float32), N)[None]
    got = _run(x, pos, cut)
    assert not S.bits(got).any()
    assert S.warp(x, pos, cut).zero.all()
