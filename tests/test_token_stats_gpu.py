"""Row statistics on the device: isi_token_stats_f32 against the float64 specification of test_token_stats_host.py,
sample.codemap_statistics / inpainting.uncertainty over it, and inpainting.resample_unlikely on top of them."""
import itertools
import math

import pytest
import torch

from test_log_probs_gpu import _rows
from test_prior_gpu import _dev, _models, _window_mask
from test_token_stats_host import spec_token_stats, tie_rows

pytestmark = pytest.mark.gpu

CLS = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}
# entropy of isi_token_stats_f32 against the float64 formula on the same fp32 logits.  The rule is test_log_probs_gpu.py's: 4x
# the largest absolute error measured on the MI355X (1.129e-06, at n = 1024; per n in test_kernel_against_float64_spec's
# docstring and in profiles/token_stats_checks.txt), far below the 1e-4 the decode kernels are held to against float64.  The
# size agrees with the arithmetic: H = log(tot) - sum e_i d_i / tot with d_i = x_i - max <= 0, e_i = expf(d_i); every e_i d_i
# carries a relative error of a few 2^-24, the two sums are wave trees plus 16 totals, and H <= ln 2048 = 7.6.
ENTROPY_TOL = 4 * 1.129e-6


def _all_rows(n, stride, g):
    """The rows of test_log_probs_gpu._rows (ordinary, one dominant logit, a token 100 nats down, logits near +-80; they need
    four classes: below that, three ordinary rows) and tie_rows (exact ties, -inf entries, an all-equal row); NaN behind the
    n classes of every row, so that a read out of the row shows."""
    if n >= 4:
        base, base_codes = _rows(n, stride, g)
    else:
        base = torch.full((3, stride), float("nan"))
        base[:, :n] = torch.randn(3, n, generator=g) * 3
        base_codes = torch.randint(0, n, (3,), generator=g)
    ties, tie_codes = tie_rows(n, g)
    logits = torch.full((base.shape[0] + ties.shape[0], stride), float("nan"))
    logits[:base.shape[0]] = base
    logits[base.shape[0]:, :n] = ties
    return logits, torch.cat([base_codes, tie_codes])


@pytest.mark.parametrize("n", [1, 32, 63, 512, 1000, 1024, 2048])
def test_kernel_against_float64_spec(n):
    """isi_token_stats_f32 at top_n = 16 on rows of stride n + 5: log_prob and top_log_probs bit-equal to
    isi_token_log_prob_f32, rank and top_codes equal to the spec exactly, entropy within ENTROPY_TOL of the float64 formula.
    Largest absolute entropy error measured on the MI355X (the test prints it), n: error --
    1: 0, 32: 2.605e-07, 63: 4.657e-07, 512: 5.752e-07, 1000: 8.641e-07, 1024: 1.129e-06, 2048: 9.040e-07."""
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    g = torch.Generator().manual_seed(1200 + n)
    logits, codes = _all_rows(n, n + 5, g)
    view = logits.to(dev)[:, :n]
    R = len(codes)
    want_lp, want_entropy, want_rank, want_top, _ = spec_token_stats(logits[:, :n], codes, 16)
    got = _ops.token_stats(view, codes.to(dev), 16)
    assert got.log_probs.dtype == got.entropy.dtype == got.top_log_probs.dtype == torch.float32
    assert got.rank.dtype == torch.int32 and got.top_codes.dtype == torch.int64
    assert got.top_codes.shape == got.top_log_probs.shape == (R, 16)
    err = float((got.entropy.cpu().double() - want_entropy).abs().max())
    print(f"token_stats n={n}: entropy max abs error {err:.3e} over {R} rows (bound {ENTROPY_TOL}); "
          f"entropies {float(want_entropy.min()):.3e} .. {float(want_entropy.max()):.4f}")
    assert torch.equal(got.log_probs, _ops.token_log_probs(view, codes.to(dev))), "log_prob differs from isi_token_log_prob_f32"
    assert torch.equal(got.rank.cpu().long(), want_rank), f"rank {got.rank.tolist()} vs spec {want_rank.tolist()}"
    assert torch.equal(got.top_codes.cpu(), want_top), "top_codes differ from the spec"
    k = min(n, 16)
    for j in range(k):
        again = _ops.token_log_probs(view, got.top_codes[:, j].contiguous())
        assert torch.equal(got.top_log_probs[:, j], again), f"top_log_probs[:, {j}] differs from isi_token_log_prob_f32"
    assert bool((got.top_log_probs[:, k:] == float("-inf")).all()) and bool((got.top_codes[:, k:] == -1).all())
    assert not torch.isnan(got.entropy).any() and bool((got.entropy >= 0).all())
    assert torch.allclose(got.log_probs.cpu().double(), want_lp, rtol=0, atol=5.2e-5)       # (test_log_probs_gpu's bound)
    assert err <= ENTROPY_TOL, f"n={n}: entropy max abs error {err:.3e}"


@pytest.mark.parametrize("n", [1, 63, 1024, 2048])
def test_out_of_range_codes_and_top_n_prefixes(n):
    """A code outside [0, n): NaN and -1 for its row, its other outputs and every other row bit-identical.  top_n = 0, 1, 5
    and 16 agree on their common prefix and on everything else; codes=None gives the same entropy and top-n."""
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    g = torch.Generator().manual_seed(1300 + n)
    logits, codes = _all_rows(n, n + 3, g)
    view, codes = logits.to(dev)[:, :n], codes.to(dev)
    full = _ops.token_stats(view, codes, 16)
    bad = codes.clone()
    bad[0], bad[2] = n, -1
    got = _ops.token_stats(view, bad, 16)
    assert torch.isnan(got.log_probs[0]) and torch.isnan(got.log_probs[2]) and got.rank[0] == -1 and got.rank[2] == -1
    keep = torch.ones(len(codes), dtype=torch.bool, device=dev)
    keep[0] = keep[2] = False
    assert torch.equal(got.log_probs[keep], full.log_probs[keep]) and torch.equal(got.rank[keep], full.rank[keep])
    assert torch.equal(got.entropy, full.entropy) and torch.equal(got.top_codes, full.top_codes)
    assert torch.equal(got.top_log_probs, full.top_log_probs)
    for top_n in (0, 1, 5):
        part = _ops.token_stats(view, codes, top_n)
        assert torch.equal(part.log_probs, full.log_probs) and torch.equal(part.entropy, full.entropy)
        assert torch.equal(part.rank, full.rank)
        if top_n == 0:
            assert part.top_codes is None and part.top_log_probs is None
        else:
            assert torch.equal(part.top_codes, full.top_codes[:, :top_n])
            assert torch.equal(part.top_log_probs, full.top_log_probs[:, :top_n])
    none = _ops.token_stats(view, None, 5)
    assert none.log_probs is None and none.rank is None
    assert torch.equal(none.entropy, full.entropy) and torch.equal(none.top_codes, full.top_codes[:, :5])
    assert torch.equal(full.rank == 0, full.top_codes[:, 0] == codes)


def test_null_outputs_are_skipped_and_nothing_else_is_written():
    """Every combination of NULL output pointers through the C entry: a passed buffer receives the full call's values, a
    sentinel-filled buffer whose pointer was withheld stays untouched (it lies in the same allocation, between the others)."""
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    n, top_n = 1000, 5
    g = torch.Generator().manual_seed(77)
    logits, codes = _all_rows(n, n + 5, g)
    logits, codes = logits.to(dev), codes.to(dev)
    R = len(codes)
    full = _ops.token_stats(logits[:, :n], codes, top_n)
    want = dict(log_prob=full.log_probs, entropy=full.entropy, rank=full.rank, top_codes=full.top_codes,
                top_log_probs=full.top_log_probs)
    fn = _hip.lib().isi_token_stats_f32
    stream = torch.cuda.current_stream().cuda_stream
    for on in itertools.product((False, True), repeat=5):
        use = dict(zip(want, on))
        # one int64 arena, the five outputs side by side in it: a write through a withheld pointer's neighbour shows
        arena = torch.full((5, R * top_n), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        bufs = {name: arena[i].view(want[name].dtype)[:want[name].numel()] for i, name in enumerate(want)}
        before = arena.clone()
        ptr = lambda name: bufs[name].data_ptr() if use[name] else None
        rc = fn(logits.data_ptr(), logits.stride(0), R, n, codes.data_ptr(), ptr("log_prob"), ptr("entropy"), ptr("rank"),
                top_n, ptr("top_codes"), ptr("top_log_probs"), stream)
        assert rc == 0, (on, _hip.lib().isi_last_error())
        torch.cuda.synchronize()
        for i, name in enumerate(want):
            if use[name]:
                got = bufs[name].reshape(want[name].shape)
                assert torch.equal(got.view(torch.int32), want[name].view(torch.int32)) if got.dtype != torch.int64 \
                    else torch.equal(got, want[name]), (on, name)
                tail = arena[i].view(torch.int8)[want[name].numel() * want[name].element_size():]
                assert bool((tail == 0x5A).all()), (on, name, "wrote behind its output")
            else:
                assert torch.equal(arena[i], before[i]), (on, name, "a withheld output was written")
    # codes == NULL: entropy and the top-n alone
    arena = torch.full((3, R * top_n), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    ent = arena[0].view(torch.float32)[:R]
    rc = fn(logits.data_ptr(), logits.stride(0), R, n, None, None, ent.data_ptr(), None, top_n, arena[1].data_ptr(),
            arena[2].view(torch.float32).data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(ent, full.entropy) and torch.equal(arena[1].reshape(R, top_n), full.top_codes)
    assert torch.equal(arena[2].view(torch.float32)[:R * top_n].reshape(R, top_n), full.top_log_probs)


# ---------------------------------------------------------------- the interface

def _case(model, seed, B):
    F, T = model.shape
    g = torch.Generator().manual_seed(seed)
    codemap = torch.randint(0, 32, (B, F, T), generator=g)
    cond = None if model.self_conditional_model else torch.randint(0, 32, (B,) + tuple(model.condition_shape), generator=g)
    mask = _window_mask(F, T, slice(1, F - 1), slice(1, 3) if T == 4 else slice(3, 6))
    return codemap, cond, mask


def _model_logits(model, codemap, cond, mask):
    """The logits [B, S, n_class] of the teacher-forced pass and the codemap / mask as sequences, from the model itself."""
    dev = _dev()
    B = codemap.shape[0]
    cls = {k: v.long().expand(B).reshape(B, 1).to(dev) for k, v in CLS.items()}
    condition = codemap if cond is None else cond
    src, tgt = model.to_sequences(codemap.to(dev), condition.to(dev), class_conditioning=cls,
                                  mask=None if mask is None else mask.to(dev))
    logits, _ = model(tgt, src)
    helper = model.target_codemaps_helper
    mask_seq = None if mask is None else helper.to_sequence(mask.to(dev)).expand(B, -1)
    return logits.contiguous(), helper.to_sequence(codemap.to(dev)).contiguous(), mask_seq


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_codemap_statistics_against_score_codemap_and_the_models_logits(golden_dir, B, masked):
    """log_probs is score_codemap's result bit for bit; the other maps are _ops.token_stats of the model's own logits,
    rearranged; outside the mask the sentinels; rank == 0 exactly where the first of top_codes is the code that is there."""
    import sample as S
    from interactive_spectrogram_inpainting.priors import _ops
    _, top, bottom = _models(golden_dir)
    dev = _dev()
    with torch.no_grad():
        for model, seed in ((top, 401), (bottom, 402)):
            codemap, cond, mask = _case(model, seed + B, B)
            mask = mask if masked else None
            kw = dict(condition=cond, class_conditioning=CLS, mask=mask)
            st = S.codemap_statistics(model, dev, codemap, top_n=4, **kw)
            score = S.score_codemap(model, dev, codemap, **kw)
            assert torch.equal(st.log_probs, score), "codemap_statistics.log_probs differs from score_codemap"
            shape = (B,) + tuple(model.shape)
            assert st.log_probs.shape == st.entropy.shape == st.rank.shape == shape
            assert st.top_codes.shape == st.top_log_probs.shape == shape + (4,)
            assert (st.entropy.dtype, st.rank.dtype, st.top_codes.dtype, st.top_log_probs.dtype) == \
                (torch.float32, torch.int32, torch.int64, torch.float32)
            logits, code_seq, mask_seq = _model_logits(model, codemap, cond, mask)
            raw = _ops.token_stats(logits, code_seq, 4)
            to_map = model.target_codemaps_helper.to_time_frequency_map
            inside = torch.ones(shape, dtype=torch.bool, device=dev) if mask is None else to_map(mask_seq)
            for name in ("log_probs", "entropy", "rank", "top_codes", "top_log_probs"):
                got, want = getattr(st, name), to_map(getattr(raw, name))
                assert torch.equal(got[inside], want[inside]), f"{name} differs from token_stats of the model's logits"
            out = ~inside
            assert bool((st.log_probs[out] == 0).all()) and bool((st.entropy[out] == 0).all())
            assert bool((st.rank[out] == -1).all()) and bool((st.top_codes[out] == -1).all())
            assert bool((st.top_log_probs[out] == float("-inf")).all())
            assert bool((st.entropy[inside] > 0).all()) and bool((st.rank[inside] >= 0).all())
            assert torch.equal((st.rank == 0) & inside, (st.top_codes[..., 0] == codemap.to(dev)) & inside)
            none = S.codemap_statistics(model, dev, codemap, **kw)                      # top_n = 0: empty last dimension
            assert none.top_codes.shape == none.top_log_probs.shape == shape + (0,)
            assert torch.equal(none.log_probs, st.log_probs) and torch.equal(none.entropy, st.entropy)
            assert torch.equal(none.rank, st.rank)


def _request(z, seed=14):
    dev = _dev()
    cls = {k[5:]: torch.from_numpy(z[k])[:1].to(dev) for k in z.files if k.startswith("cls::")}
    g = torch.Generator().manual_seed(seed)
    top_code = torch.randint(0, 32, (1, 8, 10), generator=g).to(dev)
    bottom_code = torch.randint(0, 32, (1, 16, 20), generator=g).to(dev)
    masks = {"top": _window_mask(8, 4, slice(1, 7), slice(0, 3)), "bottom": _window_mask(16, 8, slice(3, 12), slice(2, 6))}
    return cls, top_code, bottom_code, masks


@pytest.mark.parametrize("layer", ["top", "bottom"])
def test_uncertainty_is_codemap_statistics_on_the_window(golden_dir, layer):
    import inpainting as I
    import sample as S
    z, top, bottom = _models(golden_dir)
    dev = _dev()
    cls, top_code, bottom_code, masks = _request(z)
    start, mask = 3, masks[layer]
    got = I.uncertainty(top, bottom, top_code, bottom_code, mask, layer, start, cls, cls, dev, top_n=3)
    (s_top, e_top), (s_bot, e_bot), _ = I._windows(top_code, bottom_code, top, bottom, start)
    ti_top = I.make_time_indexes(s_top, top_code.shape[-1], top.shape[-1])
    ti_bot = I.make_time_indexes(s_bot, bottom_code.shape[-1], bottom.shape[-1])
    if layer == "top":
        want = S.codemap_statistics(top, dev, top_code[..., s_top:e_top], condition=top_code[..., s_top:e_top],
                                    class_conditioning=cls, mask=mask, time_indexes_source=ti_top, time_indexes_target=ti_top,
                                    top_n=3)
    else:
        want = S.codemap_statistics(bottom, dev, bottom_code[..., s_bot:e_bot], condition=top_code[..., s_top:e_top],
                                    class_conditioning=cls, mask=mask, time_indexes_source=ti_top, time_indexes_target=ti_bot,
                                    top_n=3)
    for a, b, name in zip(got, want, got._fields):
        assert torch.equal(a, b), name
    assert bool((got.log_probs[mask.to(dev)] < 0).all()) and bool((got.log_probs[~mask.to(dev)] == 0).all())
    with pytest.raises(ValueError):
        I.uncertainty(top, bottom, top_code, bottom_code, mask, "middle", start, cls, cls, dev)


@pytest.mark.parametrize("layer", ["top", "bottom"])
def test_resample_unlikely_is_timerange_change_on_the_selected_mask(golden_dir, layer):
    """The returned mask is select_unlikely of uncertainty's log-probabilities (as sequences: ties in decoding order); the
    codes are timerange_change(mask=<returned mask>) with an equally seeded generator, code for code -- a single request with
    `fraction` and with `log_prob_below`, and num_variations = 4 with return_scores; codes outside the (up-sampled) selected
    mask are the inputs'."""
    import inpainting as I
    z, top, bottom = _models(golden_dir)
    dev = _dev()
    cls, top_code, bottom_code, masks = _request(z)
    start, region = 3, masks[layer]
    model = top if layer == "top" else bottom
    helper = model.target_codemaps_helper
    lp = I.uncertainty(top, bottom, top_code, bottom_code, region, layer, start, cls, cls, dev).log_probs
    median = float(lp[region.to(dev)].median())
    args = (top, bottom, top_code, bottom_code)
    tail = (layer, start, 0.9, cls, cls, dev)
    for rule, extra in ((dict(fraction=0.3), {}), (dict(log_prob_below=median), {}),
                        (dict(fraction=0.3), dict(num_variations=4, return_scores=True)),
                        (dict(fraction=0.5), dict(num_variations=4, return_scores=True, sort_by_likelihood=True))):
        kw = dict(top_p_sampling_p=0.9, **extra)
        out = I.resample_unlikely(*args, region, *tail, generator=torch.Generator().manual_seed(91), **rule, **kw)
        selected = out[-1]
        want_sel = helper.to_time_frequency_map(I.select_unlikely(helper.to_sequence(lp), helper.to_sequence(region.to(dev)), **rule))
        assert torch.equal(selected, want_sel), (rule, "the returned mask is not the selection rule's")
        assert bool(selected.any()) and not bool((selected & ~region.to(dev)).any())
        if "fraction" in rule:
            assert int(selected.sum()) == math.ceil(rule["fraction"] * int(region.sum()))
        want = I.timerange_change(*args, selected, *tail, generator=torch.Generator().manual_seed(91), **kw)
        assert len(out) == len(want) + 1
        for a, b in zip(out[:-1], want):
            assert torch.equal(a, b), (rule, extra)
        rows = out[0].shape[0]
        assert rows == extra.get("num_variations", 1)
        full_top = torch.zeros(1, 8, 10, dtype=torch.bool, device=dev)
        full_bot = torch.zeros(1, 16, 20, dtype=torch.bool, device=dev)
        if layer == "top":
            full_top[..., start:start + 4] = selected
            full_bot = full_top.repeat_interleave(2, -2).repeat_interleave(2, -1)
        else:
            full_bot[..., 2 * start:2 * start + 8] = selected
        assert torch.equal(out[0][~full_top.expand(rows, -1, -1)], top_code.expand(rows, -1, -1)[~full_top.expand(rows, -1, -1)])
        assert torch.equal(out[1][~full_bot.expand(rows, -1, -1)], bottom_code.expand(rows, -1, -1)[~full_bot.expand(rows, -1, -1)])


def test_resample_unlikely_with_an_empty_selection_samples_nothing(golden_dir, monkeypatch):
    import inpainting as I
    z, top, bottom = _models(golden_dir)
    dev = _dev()
    cls, top_code, bottom_code, masks = _request(z)

    def refuse(*a, **k):
        raise AssertionError("an empty selection reached the sampler")
    monkeypatch.setattr(I, "sample_model", refuse)
    monkeypatch.setattr(I, "timerange_change", refuse)
    for layer in ("top", "bottom"):
        t, b, sel = I.resample_unlikely(top, bottom, top_code, bottom_code, masks[layer], layer, 3, 0.9, cls, cls, dev,
                                        log_prob_below=-1e9, generator=torch.Generator().manual_seed(1))
        assert torch.equal(t, top_code) and torch.equal(b, bottom_code) and t is not top_code
        assert sel.shape == masks[layer].shape and sel.dtype == torch.bool and not bool(sel.any())
    t, b, s, sel = I.resample_unlikely(top, bottom, top_code, bottom_code, masks["top"], "top", 3, 0.9, cls, cls, dev,
                                       fraction=0.0, num_variations=3, return_scores=True)
    assert t.shape == (3, 8, 10) and b.shape == (3, 16, 20) and torch.equal(t[2:], top_code) and torch.equal(b[:1], bottom_code)
    assert s.shape == (3,) and s.dtype == torch.float32 and bool((s == 0).all()) and not bool(sel.any())
