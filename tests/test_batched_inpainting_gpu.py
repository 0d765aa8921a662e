"""Ragged batches: independent inpainting requests decoded together, each row at its own position
(`isi_prior_sample_run_rows`).  Every row must sample what its request samples alone -- against the reference loop with
one full decoder pass per token (`_full_pass_sampling`), against `sample_model` with the request's mask shared by the
batch, and against `inpainting.timerange_change` request by request."""
import pytest
import torch

from test_prior_gpu import COMMON, FULL, _dev, _full_bottom, _full_pass_sampling, _models, _window_mask  # noqa: F401
from test_single_source_sampling_gpu import _aligned_bottom, _identity_top

pytestmark = pytest.mark.gpu

KNOBS = [("ISI_PRIOR_GRAPH", 0), ("ISI_PRIOR_GRAPH", 1), ("ISI_PRIOR_GRAPH", 3), ("ISI_PRIOR_GRAPH", 8),
         ("ISI_DECODE_NO_STAT_HANDOFF", 1)]


def _small(kind, golden_dir):
    if kind == "top":
        return _models(golden_dir)[1]
    if kind == "bottom":
        return _models(golden_dir)[2]
    if kind == "aligned_bottom":
        return _aligned_bottom(golden_dir)
    return _identity_top(golden_dir)


def _row_masks(model, B, g):
    """Row 0 full, row 1 a window, row 2 only the last token (in the target order), row 3 nothing, then windows at random
    places; built in sequence order and mapped back to [B, F, T]."""
    S = model.target_transformer_sequence_length
    seq = torch.zeros(B, S, dtype=torch.bool)
    seq[0] = True
    seq[1, S // 3:S // 3 + 9] = True
    seq[2, S - 1] = True
    for r in range(4, B):
        a = int(torch.randint(0, S - 4, (1,), generator=g))
        seq[r, a:a + int(torch.randint(1, 12, (1,), generator=g))] = True
    return model.target_codemaps_helper.to_time_frequency_map(seq).bool()


def _full_pass_row(model, init, cond, clsd, mask, uni, temperature, top_k, top_p, ti_src, ti_tgt):
    """`_full_pass_sampling` of one request with its own time indexes (given to the model's `to_sequences`)."""
    orig = model.to_sequences
    model.to_sequences = lambda *a, **k: orig(*a, time_indexes_source=ti_src, time_indexes_target=ti_tgt, **k)
    try:
        return _full_pass_sampling(model, init, cond, clsd, mask, uni, temperature, top_k, top_p)[0]
    finally:
        del model.to_sequences


@pytest.mark.parametrize("kind", ["top", "bottom", "aligned_bottom", "identity_top"])
@pytest.mark.parametrize("B", [3, 20])
def test_ragged_rows_equal_their_requests_alone(kind, B, golden_dir):
    """B = 3 (rows-in-registers kernels) and B = 20 (32-row matrix tiles): rows with different masks, temperatures,
    top-k / top-p settings, classes and time indexes; each row equals the reference loop on its request alone, under every
    graph window size and with the statistics hand-off off."""
    from interactive_spectrogram_inpainting import _hip
    import sample as S
    model = _small(kind, golden_dir)
    dev = _dev()
    g = torch.Generator().manual_seed(100 + B)
    F, T = model.shape
    init = torch.randint(0, 32, (B, F, T), generator=g)
    cond = init.clone() if model.self_conditional_model else torch.randint(0, 32, (B, 8, 4), generator=g)
    mask = _row_masks(model, B, g)
    temps = torch.tensor([0.7 + 0.1 * (r % 5) for r in range(B)])
    top_k = torch.tensor([[0, 5, 0, 3][r % 4] for r in range(B)])
    top_p = torch.tensor([[0.0, 0.0, 0.8, 0.9][r % 4] for r in range(B)])
    cls = {"pitch": torch.tensor([20 + r for r in range(B)]), "instrument_family_str": torch.full((B,), 3)}
    T_src = cond.shape[-1]
    ti_tgt = torch.stack([torch.tensor(sorted(torch.randint(0, T, (T,), generator=g).tolist())) for _ in range(B)])
    ti_src = ti_tgt if model.self_conditional_model else torch.stack(
        [torch.tensor(sorted(torch.randint(0, T_src, (T_src,), generator=g).tolist())) for _ in range(B)])
    uni = torch.rand(model.target_transformer_sequence_length, B, generator=g)
    refs = []
    for r in range(B):
        clsd = {k: v[r:r + 1].long().reshape(1, 1).to(dev) for k, v in cls.items()}
        refs.append(_full_pass_row(model, init[r:r + 1].clone().to(dev), cond[r:r + 1].to(dev), clsd, mask[r:r + 1].to(dev),
                                   uni[:, r:r + 1], float(temps[r]), int(top_k[r]), float(top_p[r]),
                                   ti_src[r:r + 1], ti_tgt[r:r + 1]).cpu())
    for name, value in KNOBS:
        with _hip.knob(name, value):
            got = S.sample_model(model, dev, B, [F, T], temps, condition=cond, class_conditioning=cls,
                                 initial_code=init.clone(), mask=mask, time_indexes_source=ti_src, time_indexes_target=ti_tgt,
                                 top_k_sampling_k=top_k, top_p_sampling_p=top_p, uniforms=uni).cpu()
        assert torch.equal(got[~mask], init[~mask]), f"{name}={value}: unmasked codes must be kept"
        for r in range(B):
            assert torch.equal(got[r], refs[r][0]), f"{name}={value}: row {r} differs from its request alone"


def test_equal_row_masks_give_the_shared_mask_codes(golden_dir):
    import sample as S
    _, _, bottom = _models(golden_dir)
    dev = _dev()
    B = 3
    g = torch.Generator().manual_seed(7)
    cond = torch.randint(0, 32, (B, 8, 4), generator=g)
    init = torch.randint(0, 32, (B, 16, 8), generator=g)
    mask = _window_mask(16, 8, slice(2, 9), slice(3, 6))
    cls = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}
    uni = torch.rand(bottom.target_transformer_sequence_length, B, generator=g)
    kw = dict(condition=cond, class_conditioning=cls, top_p_sampling_p=0.8, uniforms=uni)
    one = S.sample_model(bottom, dev, B, [16, 8], 0.9, initial_code=init.clone(), mask=mask, **kw)
    rows = S.sample_model(bottom, dev, B, [16, 8], 0.9, initial_code=init.clone(), mask=mask.expand(B, -1, -1).clone(), **kw)
    assert torch.equal(one, rows)


@pytest.mark.parametrize("B", [8, 40])
def test_ragged_bottom_prior_at_baseline_size(B):
    """The [64, 64] bottom prior: 64-token windows (32 frequencies x 2 frames) at different places.  Row r against the
    same batch sampled with request r's mask shared by every row (same kernels, same M; the prefill lengths differ, so a
    code may move where a uniform sits within rounding of a CDF step: at most 1); two rows against the reference loop.
    B = 40 runs the two-split cached attention in one workgroup."""
    import sample as S
    bottom = _full_bottom()
    dev = _dev()
    g = torch.Generator().manual_seed(31 + B)
    cond = torch.randint(0, 512, (B, 32, 32), generator=g)
    init = torch.randint(0, 512, (B, 64, 64), generator=g)
    mask = torch.cat([_window_mask(64, 64, slice(10 + (r % 3) * 8, 42 + (r % 3) * 8),
                                   slice(2 * ((5 + 7 * r) % 31), 2 * ((5 + 7 * r) % 31) + 2)) for r in range(B)])
    cls = {"pitch": torch.tensor([24]), "instrument_family_str": torch.tensor([0])}
    uni = torch.rand(bottom.target_transformer_sequence_length, B, generator=g)
    kw = dict(condition=cond, class_conditioning=cls, top_p_sampling_p=0.8, uniforms=uni)
    got = S.sample_model(bottom, dev, B, [64, 64], 1.0, initial_code=init.clone(), mask=mask, **kw).cpu()
    assert torch.equal(got[~mask], init[~mask])
    for r in range(B):
        shared = S.sample_model(bottom, dev, B, [64, 64], 1.0, initial_code=init.clone(),
                                mask=mask[r:r + 1].expand(B, -1, -1).clone(), **kw).cpu()
        moved = int((shared[r] != got[r]).sum())
        assert moved <= 1, f"row {r}: {moved} codes differ from the shared-mask call"
    clsd = {k: v.long().reshape(1, 1).to(dev) for k, v in cls.items()}
    for r in (0, B - 1):
        ref, n = _full_pass_sampling(bottom, init[r:r + 1].clone().to(dev), cond[r:r + 1].to(dev), clsd, mask[r:r + 1].to(dev),
                                     uni[:, r:r + 1], 1.0, 0, 0.8)
        assert n == 64
        moved = int((ref.cpu()[0] != got[r]).sum())
        assert moved <= 1, f"row {r}: {moved} codes differ from the reference loop"


def test_timerange_change_batch_equals_single_requests(golden_dir):
    """A codemap longer than the models' window, top and bottom requests at different start indexes, one uniform-sampling
    request: every result equals `timerange_change` of that request alone with an equally seeded generator."""
    import inpainting as I
    _, top, bottom = _models(golden_dir)
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    top_code = torch.randint(0, 32, (1, 8, 10), generator=g).to(dev)
    bottom_code = torch.randint(0, 32, (1, 16, 20), generator=g).to(dev)
    cls_t = {"pitch": torch.tensor([30]), "instrument_family_str": torch.tensor([2])}
    cls_b = {"pitch": torch.tensor([31]), "instrument_family_str": torch.tensor([4])}
    specs = [("top", 0, _window_mask(8, 4, slice(0, 8), slice(1, 3)), {}),
             ("bottom", 5, _window_mask(16, 8, slice(3, 12), slice(2, 5)), dict(top_p_sampling_p=0.8)),
             ("top", 6, _window_mask(8, 4, slice(2, 5), slice(0, 4)), dict(top_k_sampling_k=4)),
             ("bottom", 2, _window_mask(16, 8, slice(0, 16), slice(7, 8)), {}),
             ("top", 3, _window_mask(8, 4, slice(1, 7), slice(2, 3)), dict(uniform_sampling=True)),
             ("bottom", 0, _window_mask(16, 8, slice(5, 6), slice(0, 8)), dict(top_k_sampling_k=2, top_p_sampling_p=0.9))]
    requests, expected = [], []
    for i, (layer, start, m, extra) in enumerate(specs):
        base = dict(top_code=top_code, bottom_code=bottom_code, mask=m, layer=layer, start_index_top=start,
                    temperature=0.8 + 0.05 * i, class_conditioning_top=cls_t, class_conditioning_bottom=cls_b, **extra)
        requests.append(dict(base, generator=torch.Generator().manual_seed(50 + i)))
        expected.append(I.timerange_change(top, bottom, device=dev, generator=torch.Generator().manual_seed(50 + i), **base))
    got = I.timerange_change_batch(top, bottom, requests, dev)
    assert len(got) == len(specs)
    for i, ((t, b), (te, be)) in enumerate(zip(got, expected)):
        assert torch.equal(t, te), f"request {i}: top map"
        assert torch.equal(b, be), f"request {i}: bottom map"
