"""The phase-locked splice without a GPU: properties of the float64 specification (tests/spec_splice_spec.py), the experiment
that motivates it, a float32 model of the kernels inside the stated bounds, the comparison against planted faults, the host
side of `inpainting` (changed_cells, splice_weights), and every refusal of isi_spec_splice_f32 / isi_spec_splice_blend_f32
through the C ABI (the library loads without a GPU and refuses before any launch)."""
import math

import numpy as np
import pytest
import torch

import spec_splice_spec as S

PI = math.pi
HOST_CASES = [(1, 1, 5, 1, 0), (1, 2, 5, 1, 1), (3, 3, 64, 1, 0), (3, 17, 64, 3, 1), (3, 40, 130, 3, 0), (1, 40, 64, 1, 1),
              (3, 17, 1, 3, 0), (1, 17, 130, 1, 1)]                                       # B, T, F, w_batch, mel


@pytest.fixture(scope="module")
def cases():
    return {c: S.make_case(*c) for c in HOST_CASES}


# --------------------------------------------------------------------------------------------------- the specification
def test_runs_finds_every_maximal_range():
    mask = np.array([[0, 1, 1, 0, 1, 0, 0, 1], [1, 1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 1, 0, 1, 1, 0, 0]],
                    dtype=bool).T[None]                                                   # [1, T = 8, F = 4]
    t0, t1 = S.runs(mask)
    assert t0[0, [1, 2, 4, 7], 0].tolist() == [1, 1, 4, 7] and t1[0, [1, 2, 4, 7], 0].tolist() == [3, 3, 5, 8]
    assert (t0[0, :, 1] == 0).all() and (t1[0, :, 1] == 8).all()
    assert t0[0, [0, 2, 4, 5], 3].tolist() == [0, 2, 4, 4] and t1[0, [0, 2, 4, 5], 3].tolist() == [1, 3, 6, 6]


@pytest.mark.parametrize("case", HOST_CASES)
def test_continued_phase_meets_the_original_and_the_detune_is_small(cases, case):
    c = cases[case]
    s, T = c.spec, c.T
    re, im = c.xo[..., :c.F].astype(np.float64), c.xo[..., c.F:].astype(np.float64)
    phio, psi = np.arctan2(im, re), c.ph.astype(np.float64)
    n1 = s.t1 - s.t0 + 1
    inside = s.mask & s.both
    assert (np.abs(s.c[inside]) <= PI / n1[inside] + 1e-15).all()                          # |c| <= pi / (t1 - t0 + 1)
    # continue the run's formula one frame further, to t1: it must be the original's phase there, modulo 2 pi
    ia, ib = np.clip(s.t0 - 1, 0, T - 1), np.clip(s.t1, 0, T - 1)
    take = lambda x, i: np.take_along_axis(x, i, axis=1)                                   # noqa: E731
    at_t1 = take(phio, ia) + (take(psi, ib) - take(psi, ia)) + n1 * s.c
    miss = np.angle(np.exp(1j * (at_t1 - take(phio, ib))))
    assert (np.abs(miss[inside]) < 1e-9).all()
    # a right-anchored run steps into the original's phase with the decoded increment, a left-anchored one out of it
    right_only = s.mask & s.right & ~s.left
    last = right_only & (np.arange(T)[None, :, None] == s.t1 - 1)
    step = np.angle(np.exp(1j * (take(phio, ib) - s.phi - (take(psi, ib) - psi))))
    assert (np.abs(step[last]) < 1e-9).all()
    first = s.mask & s.left & (np.arange(T)[None, :, None] == s.t0)
    step = np.angle(np.exp(1j * (s.phi - take(phio, ia) - (psi - take(psi, ia)) - s.c)))
    assert (np.abs(step[first]) < 1e-9).all()
    if c.T >= 17 and c.F >= 64:                                                           # the data hold what the issue lists
        assert inside.any() and right_only.any() and (s.mask & s.left & ~s.right).any() and s.exact.any()
        assert (~s.mask).all(1).any(), "a row with no run"
        assert ((c.w > 0) & (c.w < 1)).any() and ((s.mask & (s.bound == 0)).any()), "fractional weights, a silent side"
        assert (n1[inside] == 2).any(), "runs of one frame"
        assert np.isclose(np.abs(c.ph).max(), 40 * PI, rtol=1e-2)
    assert float(s.margin.min()) >= S.WRAP_MARGIN


def test_weight_zero_returns_the_input_and_weight_one_the_plain_synthesis(cases):
    for case in HOST_CASES:
        c = cases[case]
        z = S.splice(c.xo, c.a, c.ph, np.zeros_like(c.w), c.mel)
        assert not z.mask.any() and np.array_equal(z.out, c.xo[..., :c.F].astype(np.float64) + 1j * c.xo[..., c.F:])
        o = S.splice(c.xo, c.a, c.ph, np.ones_like(c.w), c.mel)
        plain = S.synthesis_magnitude(c.a, c.mel) * np.exp(1j * c.ph.astype(np.float64))
        assert o.exact.all() and np.array_equal(o.out, plain)
        if not c.mel:                                                     # no phase arithmetic, no magnitude arithmetic
            assert np.allclose(o.bound, np.abs(plain) * (1.5 * 2.0 ** -22 + 2 * S.U), rtol=1e-12, atol=0)
        assert np.array_equal(S.splice(c.xo, c.a, c.ph, np.ones_like(c.w), c.mel, np.float32).out,
                              S.to_stft_f32_model(c.a, c.ph, c.mel))


def test_a_silent_side_under_a_fractional_weight_is_silence():
    xo = np.array([[[0.0, 3.0, 1.0, 0.0, 4.0, 1.0]]], dtype=np.float32)                    # bins 0 (silent), 3 + 4i, 1 + i
    a = np.array([[[2.0, 0.0, -1.0]]], dtype=np.float32)
    ph, w = np.zeros((1, 1, 3), dtype=np.float32), np.full((1, 1, 3), 0.5, dtype=np.float32)
    s = S.splice(xo, a, ph, w, 0)
    assert s.out.tolist() == [[[0.0, 0.0, 0.0]]] and (s.bound == 0).all()
    s = S.splice(xo, np.array([[[2.0, 4.0, 9.0]]], dtype=np.float32), ph, w, 0)
    assert s.out[0, 0, 0] == 0 and np.isclose(s.out[0, 0, 1], math.sqrt(5.0 * 4.0)) and np.isclose(s.out[0, 0, 2], math.sqrt(math.sqrt(2.0) * 9.0))


def test_blend_shares():
    for geo in S.BLEND_GEOMETRIES:
        for B in (1, 3):
            c = S.make_blend_case(*geo, B)
            s, (n_fft, hop, Tf, L) = c.spec, geo
            pos = np.arange(L) + n_fft - hop
            reach = np.stack([(pos - t * hop > 0) & (pos - t * hop < n_fft) for t in range(Tf)])          # [Tf, L]
            hits = ((c.touched != 0)[:, :, None] & reach[None]).sum(1)
            assert np.array_equal(s.g == 0, hits == 0), "g == 0 exactly where every reaching frame is untouched"
            assert (s.g[(hits == reach.sum(0)[None]) & (hits > 0)] == 1).all(), "g == 1 where all are touched"
            assert ((s.g >= 0) & (s.g <= 1)).all() and np.array_equal(s.out[s.copied], c.orig.astype(np.float64)[s.copied])


# ------------------------------------------------------------------------------------------------------ the experiment
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_locked_splice_against_the_naive_one(seed):
    locked, naive, detune = S.experiment(seed)
    print(f"seed {seed}: locked {locked:.4f} rms, naive {naive:.4f} rms, largest detune {detune:.4f} rad per frame")
    assert locked <= 0.1 * naive
    assert detune <= PI / 15


# ------------------------------------------------------------------------- the kernels' order in float32, the comparison
@pytest.mark.parametrize("case", HOST_CASES)
def test_float32_model_stays_inside_the_bound(cases, case):
    c = cases[case]
    model = S.splice(c.xo, c.a, c.ph, c.w, c.mel, np.float32).out
    assert S.compare(model, c, exact_ref=S.to_stft_f32_model(c.a, c.ph, c.mel)) <= 1.0


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_comparison_rejects_planted_faults(cases, mutant):
    for case in ((3, 17, 64, 3, 1), (3, 40, 130, 3, 0)):
        c = cases[case]
        with pytest.raises(AssertionError):
            S.compare(S.splice(c.xo, c.a, c.ph, c.w, c.mel, np.float32, mutant).out, c, mutant)


def test_comparison_rejects_a_whole_row_that_is_not_to_stft_s_bits(cases):
    c = cases[(3, 17, 64, 3, 1)]
    model, ref = S.splice(c.xo, c.a, c.ph, c.w, c.mel, np.float32).out, S.to_stft_f32_model(c.a, c.ph, c.mel)
    exact = np.concatenate([c.spec.exact, c.spec.exact], -1)
    off = np.where(exact, np.nextafter(model, np.float32(np.inf)), model)                  # one ulp: inside the bound
    S.compare(off, c)
    with pytest.raises(AssertionError):
        S.compare(off, c, exact_ref=ref)


def test_blend_model_and_its_faults():
    for geo in S.BLEND_GEOMETRIES:
        for B in (1, 3):
            c = S.make_blend_case(*geo, B)
            model = S.blend_f32_model(c.orig, c.ola, c.touched, c.n_fft, c.hop)
            assert S.compare_blend(model, c) <= 1.0
            if (~c.spec.copied).any() and (c.spec.g[~c.spec.copied] < 1).any():
                hard = np.where(c.spec.copied, c.orig, c.ola)                              # no cross-fade
                with pytest.raises(AssertionError):
                    S.compare_blend(hard, c)
            if c.spec.copied.any():
                resynth = np.where(c.spec.copied, c.orig + np.float32(1e-7) * (c.ola - c.orig), model)   # untouched samples not copied
                with pytest.raises(AssertionError):
                    S.compare_blend(resynth, c)


# ------------------------------------------------------------------------------------------------ inpainting's host side
class _Helper:
    mel = False

    def __init__(self, n_bins):
        self.n_bins = n_bins


def test_changed_cells():
    import inpainting
    top0 = torch.arange(6).reshape(1, 2, 3)
    bottom0 = torch.arange(48).reshape(1, 4, 12)                                          # 2 x 4 bottom cells under a top cell
    top1, bottom1 = top0.clone(), bottom0.clone()
    assert not inpainting.changed_cells(top0, bottom0, top1, bottom1).any()
    top1[0, 1, 2] = 99
    bottom1[0, 1, 7] = 99                                                                 # under top cell (0, 1)
    got = inpainting.changed_cells(top0, bottom0, top1, bottom1)
    assert got.dtype == torch.bool and got.tolist() == [[False, True, False], [False, False, True]]
    assert torch.equal(inpainting.changed_cells(top0[0], bottom0[0], top1[0], bottom1[0]), got)
    both = inpainting.changed_cells(torch.cat([top0, top0]), torch.cat([bottom0, bottom0]), torch.cat([top0, top1]),
                                    torch.cat([bottom0, bottom1]))
    assert both.shape == (2, 2, 3) and not both[0].any() and torch.equal(both[1], got)
    with pytest.raises(ValueError):
        inpainting.changed_cells(top0, bottom0, top1[..., :2], bottom1)
    with pytest.raises(ValueError):
        inpainting.changed_cells(top0, bottom0[..., :11], top1, bottom1[..., :11])


def test_splice_weights_rows_halo_and_ramps():
    import inpainting
    helper = _Helper(8)
    mask = torch.zeros(4, 6, dtype=torch.bool)
    mask[1, 2] = True
    w = inpainting.splice_weights(helper, mask, 12, 0, halo_top=0)                         # 2 rows and 2 frames per cell
    assert w.shape == (1, 12, 8) and w.dtype == torch.float32
    want = torch.zeros(12, 8)
    want[4:6, 2:4] = 1.0                                                                  # mask row 1 = spectrogram rows 2, 3
    assert torch.equal(w[0], want)
    w = inpainting.splice_weights(helper, mask, 12, 0, halo_top=1)                         # grown by one cell all round
    want = torch.zeros(12, 8)
    want[2:8, 0:6] = 1.0
    assert torch.equal(w[0], want)
    w = inpainting.splice_weights(helper, mask, 12, 3, halo_top=0)                         # ramps 0.75, 0.5, 0.25 on both sides
    assert w[0, :, 2].tolist() == [0, 0.25, 0.5, 0.75, 1, 1, 0.75, 0.5, 0.25, 0, 0, 0] and not w[0, :, 4].any()
    mask[1, 0] = True                                                                     # ramps of two holes: the larger wins
    w = inpainting.splice_weights(helper, mask, 12, 3, halo_top=0)
    assert w[0, :, 2].tolist() == [1, 1, 0.75, 0.75, 1, 1, 0.75, 0.5, 0.25, 0, 0, 0]
    edge = torch.zeros(4, 6, dtype=torch.bool)
    edge[3, 5] = True                                                                     # the halo stops at the map's edge
    w = inpainting.splice_weights(helper, edge, 6, 0, halo_top=1)
    assert w.shape == (1, 6, 8) and bool((w[0, 4:, 4:] == 1).all()) and float(w.sum()) == 2 * 4
    batch = torch.stack([mask, edge])
    assert inpainting.splice_weights(helper, batch, 12, 1).shape == (2, 12, 8)
    assert not inpainting.splice_weights(helper, torch.zeros(4, 6, dtype=torch.bool), 12, 5).any()
    for bad in (dict(n_frames=13), dict(feather_frames=-1), dict(halo_top=-1)):
        with pytest.raises(ValueError):
            inpainting.splice_weights(helper, mask, **dict(dict(n_frames=12, feather_frames=1, halo_top=1), **bad))
    with pytest.raises(ValueError):
        inpainting.splice_weights(_Helper(9), mask, 12, 1)


def test_splice_weights_bring_mel_rows_to_linear_bins():
    import inpainting
    from GANsynth_pytorch.spectrograms_helper import MelSpectrogramsHelper
    helper = MelSpectrogramsHelper(fs_hz=16000, n_fft=64, hop_length=16, window_length=64)
    M = helper._mel_matrix()                                                               # [linear, mel]
    mask = torch.zeros(4, 3, dtype=torch.bool)
    mask[2, 1] = True                                                                     # mel bands 16 .. 23, frames 2, 3
    w = inpainting.splice_weights(helper, mask, 6, 0, halo_top=0)
    assert w.shape == (1, 6, 32) and not w[0, [0, 1, 4, 5]].any() and torch.equal(w[0, 2], w[0, 3])
    band = torch.zeros(32, dtype=torch.float64)
    band[16:24] = 1.0
    fed = M.sum(1)
    want = torch.where(fed > 0, (M @ band) / torch.where(fed > 0, fed, torch.ones_like(fed)), torch.zeros_like(fed))
    assert torch.allclose(w[0, 2].double(), want, atol=1e-7)
    feeds = (M[:, 16:24] > 0).any(1)
    assert torch.equal(w[0, 2] > 0, feeds) and feeds.any() and not feeds.all()             # > 0 exactly where a bin feeds a masked band
    only = feeds & ~(M[:, :16] > 0).any(1) & ~(M[:, 24:] > 0).any(1)
    assert bool((w[0, 2][only] == 1).all())
    full = inpainting.splice_weights(helper, torch.ones(4, 3, dtype=torch.bool), 6, 0, halo_top=0)
    assert bool((full[0][:, fed > 0] == 1).all()) and not full[0][:, fed == 0].any()


def test_get_audio_spliced_route_refuses_without_touching_the_gpu():
    import io
    import flask_server
    from GANsynth_pytorch.spectrograms_helper import SpectrogramsHelper
    helper = SpectrogramsHelper(fs_hz=16000, n_fft=128, hop_length=32, window_length=128)
    wav = flask_server._wav_bytes(torch.sin(torch.arange(640) * 0.1) * 0.5, 16000)
    codes = '{"top_code": [[0]], "bottom_code": [[0]]}'
    post = lambda client, **data: client.post('/get-audio-spliced', data=data, content_type='multipart/form-data')   # noqa: E731
    client = flask_server.create_app(None, None, None, {}, "cpu", spectrograms_helper=helper).test_client()
    assert post(client, codes=codes).status_code == 400                                    # no audio part
    assert post(client, audio=(io.BytesIO(b"not a wave file"), 'a.wav'), codes=codes).status_code == 400
    assert post(client, audio=(io.BytesIO(wav), 'a.wav')).status_code == 400               # no codes part
    assert post(client, audio=(io.BytesIO(wav), 'a.wav'), codes='{"top_code": [[0]]}').status_code == 400
    assert post(client, audio=(io.BytesIO(wav), 'a.wav'), codes='not json').status_code == 400
    assert client.get('/get-audio-spliced').status_code == 405
    no_helper = flask_server.create_app(None, None, None, {}, "cpu").test_client()
    assert post(no_helper, audio=(io.BytesIO(wav), 'a.wav'), codes=codes).status_code == 501


# ------------------------------------------------------------------------------------------ refusals before any launch
def test_entry_points_refuse_bad_arguments_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    ok = 0x10000                     # non-null, never dereferenced on the host
    INVALID, UNSUPPORTED = -1, -4

    def refused(rc, message, code=INVALID):
        assert rc == code
        assert message in L.isi_last_error(), L.isi_last_error()

    good = dict(stft_orig=ok, a=ok, ph=ok, w=ok, w_batch=1, stft_out=ok, B=2, T=5, F=3, mel=0)

    def splice(**change):
        g = dict(good, **change)
        return L.isi_spec_splice_f32(g["stft_orig"], g["a"], g["ph"], g["w"], g["w_batch"], g["stft_out"], g["B"], g["T"], g["F"],
                                     g["mel"], None)

    for name in ("stft_orig", "a", "ph", "w", "stft_out"):
        refused(splice(**{name: None}), b"spec_splice: null pointer")
    for name in ("B", "T", "F"):
        for v in (0, -1):
            refused(splice(**{name: v}), b"spec_splice: B, T and F must be at least 1")
    for v in (0, 3, -1):
        refused(splice(w_batch=v), b"spec_splice: w_batch must be 1 or B")
    for v in (2, -1):
        refused(splice(mel=v), b"spec_splice: mel must be 0 or 1")
    span = b"spec_splice: B must stay below 65536, T below 524281 and B T F below 2^59"
    refused(splice(B=65536, w_batch=65536), span, UNSUPPORTED)
    refused(splice(T=524281), span, UNSUPPORTED)
    refused(splice(B=1 << 15, w_batch=1, T=1 << 19, F=1 << 25), span, UNSUPPORTED)       # exactly 2^59
    refused(splice(B=65535, w_batch=1, T=524280, F=(1 << 31) - 1), span, UNSUPPORTED)

    good_b = dict(orig=ok, ola=ok, touched=ok, out=ok, B=2, T_frames=7, n_fft=16, hop=4, L=16)

    def blend(**change):
        g = dict(good_b, **change)
        return L.isi_spec_splice_blend_f32(g["orig"], g["ola"], g["touched"], g["out"], g["B"], g["T_frames"], g["n_fft"], g["hop"],
                                           g["L"], None)

    for name in ("orig", "ola", "touched", "out"):
        refused(blend(**{name: None}), b"spec_splice_blend: null pointer")
    for name in ("B", "T_frames", "L"):
        for v in (0, -1):
            refused(blend(**{name: v}), b"spec_splice_blend: B, T_frames and L must be at least 1")
    for change in (dict(hop=5), dict(hop=0), dict(hop=-4), dict(n_fft=0), dict(hop=32), dict(n_fft=-16)):
        refused(blend(**change), b"spec_splice_blend: hop must be positive and divide n_fft")
    span = b"spec_splice_blend: B must stay below 65536 and L below 2^39"
    refused(blend(B=65536), span, UNSUPPORTED)
    refused(blend(L=1 << 39), span, UNSUPPORTED)
    refused(blend(L=1 << 62), span, UNSUPPORTED)
