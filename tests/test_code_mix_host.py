"""Per-cell mixtures of codes without a GPU: the float64 specification (tests/code_mix_spec.py) against the plain torch
expression and against its own rules, an fp32 model of the kernel's order inside the stated bound, the GPU file's
comparison against planted faults, every refusal of isi_embed_mix_f32 (the library loads without a GPU and refuses before
any launch), and `inpainting.morph`'s weight handling on a stub VQ-VAE."""
from types import SimpleNamespace

import pytest
import torch

import code_mix_spec as S

NAN = float("nan")


# --------------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("M,N,D,K", [(1, 5, 4, 3), (2, 33, 12, 7), (3, 64, 8, 512), (8, 19, 64, 16)])
def test_spec_equals_the_torch_expression_on_valid_inputs(M, N, D, K):
    g = torch.Generator().manual_seed(M * 100 + N)
    E = torch.randn(K, D, generator=g)
    ids = torch.randint(0, K, (M, N), generator=g)
    w = torch.randn(M, N, generator=g)
    w[w == 0] = 1.0
    mix, mag, terms, bad = S.mix_spec(ids, w, E)
    want = (w.double()[..., None] * E.double()[ids]).sum(0)
    assert not bad.any() and bool((terms == M).all())
    assert bool(((mix - want).abs() <= 2.0 ** -50 * mag).all())          # the same float64 products in another order
    assert torch.allclose(mag, (w.double()[..., None] * E.double()[ids]).abs().sum(0), rtol=1e-14, atol=0)


def test_spec_zero_weights_hide_ids_and_rows():
    E = torch.tensor([[1.0, -2.0, 0.0, -0.0], [NAN] * 4, [3.0, 4.0, 5.0, 6.0]])
    K = 3
    #               cell 0      1       2        3            4      5
    ids = torch.tensor([[0, -1, 1, S.BIG, 2, K],
                        [2, 2, 2, S.MASK_TOKEN, 1, -1]])
    w = torch.tensor([[0.5, 0.0, -0.0, 0.0, 1.0, -0.0],
                      [0.25, 2.0, 1.0, -0.0, 0.0, 0.0]])
    mix, mag, terms, bad = S.mix_spec(ids, w, E)
    assert not bad.any() and terms.tolist() == [2, 1, 1, 0, 1, 0]
    assert torch.equal(mix[0], 0.5 * E[0].double() + 0.25 * E[2].double())
    assert torch.equal(mix[1], 2.0 * E[2].double())                      # -1 under +0.0 is never looked at
    assert torch.equal(mix[2], E[2].double())                            # the NaN row under -0.0 is never read
    for cell in (3, 5):                                                   # no term: -0.0
        assert bool((mix[cell] == 0).all()) and bool(torch.signbit(mix[cell]).all())
    assert torch.equal(mix[4], E[2].double()) and bool((mag[3] == 0).all())
    one_hot = mix[4].float()
    assert torch.equal(S.bits(one_hot), S.bits(E[2]))
    mix0 = S.mix_spec(torch.tensor([[0]]), torch.tensor([[1.0]]), E)[0]  # weight 1 over a row with -0.0 keeps the sign
    assert torch.equal(S.bits(mix0.float()), S.bits(E[:1]))


def test_spec_bad_ids_make_their_cell_nan_and_only_it():
    E = torch.arange(12.0).reshape(3, 4)
    ids = torch.tensor([[0, -1, 1, 3, 2, S.BIG],
                        [1, 1, 3, 1, 2, 0]])
    w = torch.tensor([[1.0, 0.5, 1.0, NAN, 1.0, 1e-30],
                      [1.0, 0.5, 0.0, 0.0, 1.0, 0.0]])
    mix, _, terms, bad = S.mix_spec(ids, w, E)
    assert bad.tolist() == [False, True, False, True, False, True]       # cell 2: the bad id sits under a zero weight
    assert torch.equal(torch.isnan(mix).all(-1), bad) and torch.equal(torch.isnan(mix).any(-1), bad)
    assert terms.tolist() == [2, 2, 1, 1, 2, 1]                          # a NaN weight is a term


# ------------------------------------------------------------------------------- the kernel's order, and the comparison
CASES = [(17, 1, 4, 3), (17, 2, 12, 1), (257, 3, 12, 512), (257, 8, 64, 512), (1031, 2, 64, 3), (1, 3, 4, 512)]


@pytest.mark.parametrize("N,M,D,K", CASES)
def test_fp32_model_of_the_kernel_stays_inside_the_bound(N, M, D, K):
    case = S.make_case(N, M, D, K)
    if N >= 17:
        assert len(case.bad_cells) == 3
        _, _, terms, bad = S.mix_spec(case.ids, case.weights, case.E)
        assert bad.nonzero().flatten().tolist() == case.bad_cells and bool((terms == 0).any())
        hidden = case.ids[case.weights == 0]
        wanted = {-1, K, S.BIG} | ({case.nan_row} if case.nan_row is not None else set())
        assert wanted <= set(hidden.tolist()), "every kind of hidden id sits under a zero weight"
        assert bool(torch.signbit(case.weights[case.weights == 0]).any()) and not bool(torch.signbit(case.weights[case.weights == 0]).all())
        if case.nan_row is not None:
            assert not bool(((case.ids == case.nan_row) & (case.weights != 0)).any())
    ratio = S.compare(S.model_f32(case), case, f"model N={N} M={M} D={D} K={K}")
    assert ratio <= 1.0


def test_fp32_model_inside_the_bound_where_everything_cancels():
    """weights +w, -w over the same row, then a third term 2^-20 as large: the result is rounding error plus a small term,
    the bound stays relative to the absolute sum"""
    g = torch.Generator().manual_seed(5)
    N, D, K = 64, 8, 16
    E = torch.randn(K, D, generator=g)
    ids = torch.randint(0, K, (3, N), generator=g)
    ids[1] = ids[0]
    w = torch.randn(3, N, generator=g)
    w[1] = -w[0]
    w[2] *= 2.0 ** -20
    case = SimpleNamespace(N=N, M=3, D=D, K=K, E=E, ids=ids, weights=w, ids_buf=ids.reshape(-1), ids_stride=N,
                           w_buf=w.reshape(-1), w_stride=N)
    assert S.compare(S.model_f32(case), case, "cancelling") <= 1.0


@pytest.mark.parametrize("fault", ["drop_term", "shifted_weights", "zero_not_skipped", "clamped_id", "nan_leak",
                                   "stride_ignored", "plus_zero"])
def test_comparison_rejects_planted_faults(fault):
    for N, M, D, K in ((257, 3, 12, 512), (17, 2, 4, 3)):
        case = S.make_case(N, M, D, K)
        assert S.compare(S.model_f32(case), case) <= 1.0
        with pytest.raises(AssertionError):
            S.compare(S.model_f32(case, fault), case, fault)


# ------------------------------------------------------------------------------------------ refusals before any launch
def test_embed_mix_refuses_bad_arguments_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    L = _hip.lib()
    ok, odd = 0x10000, 0x10004        # non-null, never dereferenced on the host: 16-byte aligned / 4 bytes off
    INVALID, UNSUPPORTED = -1, -4
    good = dict(ids=ok, ids_stride=10, weights=ok, w_stride=10, codes=ok, out=ok, ldo=8, N=10, M=2, D=8, K=4)

    def call(**change):
        a = dict(good, **change)
        return L.isi_embed_mix_f32(a["ids"], a["ids_stride"], a["weights"], a["w_stride"], a["codes"], a["out"], a["ldo"], a["N"],
                                   a["M"], a["D"], a["K"], None)

    def refused(rc, message, code=INVALID):
        assert rc == code
        assert message in L.isi_last_error(), L.isi_last_error()

    for name in ("ids", "weights", "codes", "out"):
        refused(call(**{name: None}), b"embed_mix: null pointer")
    for N in (0, -3):
        refused(call(N=N), b"embed_mix: N must be positive")
    for M in (0, 9, -1):
        refused(call(M=M), b"embed_mix: M must be 1..8")
    for D in (0, -4, 6, 7):
        refused(call(D=D), b"embed_mix: D must be a positive multiple of 4")
    for K in (0, -1):
        refused(call(K=K), b"embed_mix: K must be positive")
    aligned = b"embed_mix: codes and out must be 16-byte aligned and ldo a multiple of 4"
    refused(call(codes=odd), aligned)
    refused(call(out=odd), aligned)
    refused(call(ldo=10), aligned)
    refused(call(ldo=4), b"embed_mix: ldo must be at least D")
    strides = b"embed_mix: ids_stride and w_stride must be at least N"
    refused(call(ids_stride=9), strides)
    refused(call(w_stride=9), strides)
    refused(call(w_stride=-10), strides)
    # spans beyond the kernel's index arithmetic: N D / 4 lanes in 32 bits, compared with >= (2^31 itself would wrap)
    span = b"embed_mix: N D / 4 must stay below 2^31"
    big = 1 << 29
    refused(call(N=big, D=16, ldo=16, ids_stride=big, w_stride=big), span, UNSUPPORTED)       # exactly 2^31 lanes
    refused(call(N=1 << 31, D=4, ldo=4, ids_stride=1 << 31, w_stride=1 << 31), span, UNSUPPORTED)
    refused(call(N=1 << 40, D=4, ldo=4, ids_stride=1 << 40, w_stride=1 << 40), span, UNSUPPORTED)
    refused(call(ids_stride=1 << 56), span, UNSUPPORTED)
    refused(call(w_stride=1 << 56), span, UNSUPPORTED)
    refused(call(ldo=1 << 31), span, UNSUPPORTED)


# ------------------------------------------------------------------------------------------ morph on a stub VQ-VAE
class _Stub:
    """records what reaches VQVAE.decode_code_mix"""

    def __init__(self, K=16):
        self.quantize_t = SimpleNamespace(n_embed=K)
        self.quantize_b = SimpleNamespace(n_embed=K)
        self.calls = []

    def decode_code_mix(self, codes_t, weights_t, codes_b, weights_b):
        self.calls.append((codes_t, weights_t, codes_b, weights_b))
        return "spectrogram"


F_T, T_T, F_B, T_B = 2, 3, 4, 12          # frequency ratio 2, time ratio 4


def _sounds(M, K=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, K, (1, F_T, T_T), generator=g), torch.randint(0, K, (1, F_B, T_B), generator=g)) for _ in range(M)]


def _under(w_top):
    return w_top.repeat_interleave(F_B // F_T, -2).repeat_interleave(T_B // T_T, -1)


def test_morph_weight_forms_and_their_expansion_to_the_bottom_map():
    import inpainting
    sounds = _sounds(3)
    stub = _Stub()
    # M scalars
    assert inpainting.morph(stub, sounds, [0.5, 0.25, 0.25]) == "spectrogram"
    ct, wt, cb, wb = stub.calls[-1]
    assert ct.shape == (3, 1, F_T, T_T) and cb.shape == (3, 1, F_B, T_B) and ct.dtype == cb.dtype == torch.int64
    assert all(torch.equal(ct[m], sounds[m][0]) and torch.equal(cb[m], sounds[m][1]) for m in range(3))
    assert wt.dtype == wb.dtype == torch.float32 and wt.shape == ct.shape and wb.shape == cb.shape
    for m, v in enumerate((0.5, 0.25, 0.25)):
        assert bool((wt[m] == v).all()) and bool((wb[m] == v).all())
    # [M, T_top]: a morph that moves in time
    a = torch.tensor([1.0, 0.5, 0.0])
    per_column = torch.stack([a, 1 - a, torch.zeros(3)])
    inpainting.morph(stub, sounds, per_column)
    _, wt, _, wb = stub.calls[-1]
    assert torch.equal(wt[:, 0], per_column[:, None, :].expand(3, F_T, T_T))
    assert torch.equal(wb[:, 0], _under(wt[:, 0])) and wb[0, 0, 3, 4:8].tolist() == [0.5] * 4
    # [M, F_top, T_top]
    g = torch.Generator().manual_seed(3)
    full = torch.rand(3, F_T, T_T, generator=g, dtype=torch.float64)
    full = (full / full.sum(0)).float()
    inpainting.morph(stub, sounds, full)
    _, wt, _, wb = stub.calls[-1]
    assert torch.equal(wt[:, 0], full) and torch.equal(wb[:, 0], _under(full))
    # the bottom map's own weights
    bottom = torch.zeros(3, F_B, T_B)
    bottom[2] = 1.0
    inpainting.morph(stub, sounds, [1.0, 0.0, 0.0], weights_bottom=bottom)
    _, wt, _, wb = stub.calls[-1]
    assert bool((wt[0] == 1).all()) and torch.equal(wb[:, 0], bottom)
    # a batch of sounds: the same weights for every row
    batch = [(t.expand(2, -1, -1), b.expand(2, -1, -1)) for t, b in sounds]
    inpainting.morph(stub, batch, per_column)
    ct, wt, _, wb = stub.calls[-1]
    assert ct.shape == (3, 2, F_T, T_T) and torch.equal(wt[:, 0], wt[:, 1]) and torch.equal(wb[:, 1], _under(wt[:, 0]))


def test_morph_refuses_weights_that_are_not_convex():
    import inpainting
    sounds, stub = _sounds(2), _Stub()
    for bad in ([0.5, 0.6], [1.5, -0.5], [NAN, 1.0], [float("inf"), 0.0], [0.5, 0.5 + 3e-6], [1.0], [0.2, 0.3, 0.5],
                torch.full((2, T_T + 1), 0.5), torch.full((2, F_B, T_T), 0.5), torch.full((2, 1, 1, 1), 0.5)):
        with pytest.raises(ValueError):
            inpainting.morph(stub, sounds, bad)
    per_column = torch.full((2, T_T), 0.5)
    per_column[0, 1] = 0.4                                               # one column does not sum to 1
    with pytest.raises(ValueError):
        inpainting.morph(stub, sounds, per_column)
    with pytest.raises(ValueError):
        inpainting.morph(stub, sounds, [0.5, 0.5], weights_bottom=torch.full((2, F_T, T_T), 0.5))
    with pytest.raises(ValueError):
        inpainting.morph(stub, sounds, [0.5, 0.5], weights_bottom=[0.5, 0.6])
    with pytest.raises(ValueError):
        inpainting.morph(stub, _sounds(9), [1 / 9] * 9)
    with pytest.raises(ValueError):
        inpainting.morph(stub, [], [])
    with pytest.raises(ValueError):                                      # unequal shapes
        inpainting.morph(stub, [sounds[0], (sounds[1][0][..., :2], sounds[1][1][..., :8])], [0.5, 0.5])
    assert not stub.calls
    inpainting.morph(stub, sounds, [0.5, 0.5 + 5e-7])                     # inside the 1e-6 of the sum
    assert len(stub.calls) == 1


def test_morph_raises_index_error_only_under_a_non_zero_weight():
    import inpainting
    K = 16
    stub = _Stub(K)
    (ta, ba), (tb, bb) = _sounds(2, K)
    masked_t, masked_b = tb.clone(), bb.clone()
    masked_t[0, 0, 2], masked_b[0, 1, 8:12] = K, -1                      # a mask token / the search's -1 in the last top column
    col = torch.tensor([[1.0, 0.5, 1.0], [0.0, 0.5, 0.0]])               # ... which source b does not take part in
    assert inpainting.morph(stub, [(ta, ba), (masked_t, masked_b)], col) == "spectrogram"
    with pytest.raises(IndexError, match="top"):
        inpainting.morph(stub, [(ta, ba), (masked_t, bb)], [0.5, 0.5])
    with pytest.raises(IndexError, match="bottom"):
        inpainting.morph(stub, [(ta, ba), (tb, masked_b)], [0.5, 0.5])
    with pytest.raises(IndexError, match="bottom"):                      # the bottom map's own weights reach the bad cells
        inpainting.morph(stub, [(ta, ba), (tb, masked_b)], col, weights_bottom=[0.5, 0.5])
    assert len(stub.calls) == 1


def test_crossfade_and_sweep_weights_on_the_stub():
    import inpainting
    stub = _Stub()
    a, b = _sounds(2)
    inpainting.crossfade(stub, a, b, 1, 0)                               # the hard cut: one-hot maps
    _, wt, _, wb = stub.calls[-1]
    assert wt[1, 0, 0].tolist() == [0.0, 1.0, 1.0] and wt[0, 0, 0].tolist() == [1.0, 0.0, 0.0]
    assert wb[1, 0, 0].tolist() == [0.0] * 4 + [1.0] * 8
    inpainting.crossfade(stub, a, b, 1, 1)                               # one top column, four bottom columns of ramp
    _, wt, _, wb = stub.calls[-1]
    assert wt[1, 0, 0].tolist() == [0.0, 0.5, 1.0]
    assert torch.allclose(wb[1, 0, 0], torch.tensor([0.0] * 4 + [0.2, 0.4, 0.6, 0.8] + [1.0] * 4))
    assert torch.allclose(wt.sum(0), torch.ones(1)) and torch.allclose(wb.sum(0), torch.ones(1))
    for start, width in ((-1, 1), (2, 2), (0, -1)):
        with pytest.raises(ValueError):
            inpainting.crossfade(stub, a, b, start, width)
    inpainting.morph_sweep(stub, a, b, 5)
    ct, wt, cb, wb = stub.calls[-1]
    assert ct.shape == (2, 5, F_T, T_T) and cb.shape == (2, 5, F_B, T_B)
    alpha = torch.linspace(0, 1, 5)
    assert torch.equal(wt[1, :, 0, 0], alpha) and torch.equal(wt[0, :, 1, 2], 1 - alpha) and torch.equal(wb[1, :, 3, 11], alpha)
    assert torch.equal(ct[0, 3], a[0][0]) and torch.equal(cb[1, 4], b[1][0])
    for steps in (0, 257):
        with pytest.raises(ValueError):
            inpainting.morph_sweep(stub, a, b, steps)
