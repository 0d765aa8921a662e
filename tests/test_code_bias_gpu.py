"""Code palettes and logit bias in prior sampling, on the GPU: the BIAS instantiations of the draw kernel against the float64
specification on float32(logits + bias) (`isi_sample_row_bias_f32`), the choice of the bias row per launch row, and the
decode loop's addressing of `isi_prior_code_bias.code_bias_index` -- by token, per batch row, in sequence order -- in every
form of the loop, through `sample_model(code_bias / code_bias_map / allowed_codes)` and `inpainting.timerange_change`.
With the options off nothing changes; a zero bias draws what the call without it draws."""
import contextlib
import time

import numpy as np
import pytest
import torch

import tests_support as TS
from test_code_bias_host import NEG, TOP_U, biased_cases
from test_prior_gpu import _close, _dev, _models, _window_mask

pytestmark = pytest.mark.gpu

CLS = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}
LOOP_TOL = 2e-4            # tests/test_log_probs_gpu.py: in-loop against teacher-forced log-probabilities
CHUNK = 32768              # rows per launch, at most


# ---------------------------------------------------------------- the draw kernel

def _device_rows(logits, stride, rows, dev):
    """[rows, n] view of a [rows, stride] buffer: the logits in every row, NaN behind them."""
    buf = torch.full((rows, stride), float("nan"), dtype=torch.float32, device=dev)
    view = buf[:, :logits.shape[0]]
    view.copy_(torch.from_numpy(logits).to(dev).expand_as(view))
    return view


def _device_table(bias, dev):
    """[2, n] view of a [2, n + 3] table: row 0 all NaN (reading the wrong row shows), row 1 the bias, NaN behind it."""
    n = bias.shape[0]
    buf = torch.full((2, n + 3), float("nan"), dtype=torch.float32, device=dev)
    buf[1, :n] = torch.from_numpy(bias).to(dev)
    return buf[:, :n]


@pytest.mark.parametrize("n", [2, 64, 65, 513, 1024])
def test_biased_draw_against_float64_spec(n):
    """Every case of TS.sampling_cases(n) crossed with the six bias rows of tests/test_code_bias_host.py (zeros, a random
    half-banned palette, a palette of one class, a dense 3 * randn bias, +20 on the row's lowest class, the argmax banned),
    the top_p picked again for the biased row; logit stride n or n + 5 and table stride n + 3, NaN behind both.
    `filtered` equals the specification of float32(logits + bias) exactly -- kept mask, and kept values
    float32(logits + bias) * float32(1 / T) bit for bit --; every draw at u = 0, at the largest float32 below 1 and on the
    boundary sweep of the biased specification passes TS.sampling_accepts at TS.SAMPLING_TAU.  No draw is a banned class,
    the one-class palette draws its class for every u, and a zero bias draws what isi_sample_row_f32 draws."""
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    t0 = time.perf_counter()
    cases, generated = biased_cases(n)
    assert len(cases) >= 0.9 * generated
    bad, rows_checked = [], 0
    for c, kind, bias, biased in cases:
        spec = TS.sampling_spec(biased, c.temperature, c.top_k, c.top_p)
        tag = f"{c.name} T={c.temperature} k={c.top_k} p={c.top_p!r} bias={kind}"
        table = _device_table(bias, dev)
        one = torch.ones(2, dtype=torch.int32)
        _, filt = _ops.sample_rows(_device_rows(c.logits, c.stride, 2, dev), c.temperature, c.top_k, c.top_p,
                                   torch.tensor([0.25, 0.75]), return_filtered=True, bias=table, bias_rows=one)
        filt = filt.cpu().numpy()
        want = np.where(spec.kept, spec.lg, NEG).astype(np.float32)
        for r in range(2):
            if not np.array_equal(np.isfinite(filt[r]), spec.kept):
                bad.append(f"{tag}: kept mask differs at classes {np.flatnonzero(np.isfinite(filt[r]) != spec.kept)[:8].tolist()}")
            elif not np.array_equal(filt[r].view(np.int32), want.view(np.int32)):
                bad.append(f"{tag}: kept values are not float32(logits + bias) * float32(1 / T) bit for bit")
        u_sw, _ = TS.sampling_sweep_uniforms(spec)
        u = np.concatenate([np.array([0.0, TOP_U], dtype=np.float32), u_sw])
        toks = []
        for i in range(0, u.shape[0], CHUNK):
            uc = torch.from_numpy(u[i:i + CHUNK]).to(dev)
            view = _device_rows(c.logits, c.stride, uc.shape[0], dev)
            tok = _ops.sample_rows(view, c.temperature, c.top_k, c.top_p, uc, bias=table,
                                   bias_rows=torch.ones(uc.shape[0], dtype=torch.int32))
            if kind == "zeros" and not torch.equal(tok, _ops.sample_rows(view, c.temperature, c.top_k, c.top_p, uc)):
                bad.append(f"{tag}: a zero bias draws other tokens than the entry without a bias")
            toks.append(tok)
        tok = torch.cat(toks).cpu().numpy()
        rows_checked += tok.shape[0]
        ok, first, last = TS.sampling_accepts(spec, u, tok)
        for i in np.flatnonzero(~ok)[:3]:
            bad.append(f"{tag}: u={u[i]!r} drew class {tok[i]} ({'kept' if spec.kept[tok[i]] else 'NOT KEPT'}); accepted: "
                       f"non-zero classes {first[i]} .. {last[i]} ({int((~ok).sum())} such draws in this case)")
        if (bias[tok] == NEG).any():
            bad.append(f"{tag}: drew a banned class, e.g. {tok[bias[tok] == NEG][:4].tolist()}")
        if kind == "one_class" and not (tok == int(np.flatnonzero(bias == 0.0)[0])).all():
            bad.append(f"{tag}: the palette of one class drew another class")
    print(f"n={n}: {len(cases)} of {generated} biased cases, {rows_checked} draws, {len(bad)} findings, "
          f"{time.perf_counter() - t0:.1f} s")
    assert not bad, f"{len(bad)} findings, the first:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("temperature,top_k,top_p", [(1.0, 0, 0.0), (0.7, 5, 0.0), (0.9, 40, 0.8)])
def test_bias_row_selection_per_launch_row(temperature, top_k, top_p):
    """A 3-row table and bias_row mixing -1, 0, 2 and out-of-range values over 8 launch rows of different logits: every
    row's draw and filtered row equal a one-row call with that bias row; -1 and out-of-range equal a call with no bias and
    read nothing (the table has three rows; the indices reach far beyond it on both sides)."""
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    n = 513
    g = torch.Generator().manual_seed(61)
    logits = torch.full((8, n + 5), float("nan"))
    logits[:, :n] = 3.0 * torch.randn(8, n, generator=g)
    table = torch.full((3, n + 3), float("nan"))
    table[:, :n] = 3.0 * torch.randn(3, n, generator=g)
    table[2, :n][torch.rand(n, generator=g) < 0.5] = -float("inf")
    table[2, 7] = 0.0
    index = torch.tensor([-1, 0, 2, 3, 2, 0, 2 ** 31 - 1, -2 ** 31], dtype=torch.int64)
    u = torch.rand(8, generator=g)
    view, tv = logits.to(dev)[:, :n], table.to(dev)[:, :n]
    tok, filt = _ops.sample_rows(view, temperature, top_k, top_p, u, return_filtered=True, bias=tv,
                                 bias_rows=index.to(torch.int32))
    differ = 0
    for r in range(8):
        i = int(index[r])
        kw = dict(bias=tv[i]) if 0 <= i < 3 else {}
        t1, f1 = _ops.sample_rows(view[r:r + 1], temperature, top_k, top_p, u[r:r + 1], return_filtered=True, **kw)
        assert torch.equal(tok[r:r + 1], t1), f"row {r} (bias row {i}): token"
        assert torch.equal(filt[r:r + 1], f1), f"row {r} (bias row {i}): filtered logits"
        plain = _ops.sample_rows(view[r:r + 1], temperature, top_k, top_p, u[r:r + 1], return_filtered=True)[1]
        differ += int(not torch.equal(f1, plain))
    assert differ == 4, "the biased rows must differ from the unbiased ones for the comparison to mean anything"
    # no index row: table row 0 on every launch row
    t0, f0 = _ops.sample_rows(view, temperature, top_k, top_p, u, return_filtered=True, bias=tv)
    tz, fz = _ops.sample_rows(view, temperature, top_k, top_p, u, return_filtered=True, bias=tv, bias_rows=torch.zeros(8))
    assert torch.equal(t0, tz) and torch.equal(f0, fz)


# ---------------------------------------------------------------- the loop

def _request(model, seed, B=1):
    F, T = model.shape
    g = torch.Generator().manual_seed(seed)
    init = torch.randint(0, 32, (B, F, T), generator=g)
    cond = None if model.self_conditional_model else torch.randint(0, 32, (B,) + tuple(model.condition_shape), generator=g)
    return init, cond, g


def _sample(model, B, uni, init, cond, mask, kv=None, N=None, temperature=0.8, top_k=5, top_p=0.9, **kw):
    import sample as S
    return S.sample_model(model, _dev(), B, list(model.shape), temperature=temperature, condition=cond,
                          class_conditioning=CLS, initial_code=init.clone(), mask=mask, top_k_sampling_k=top_k,
                          top_p_sampling_p=top_p, uniforms=uni, kv_cache_dtype=kv, num_variations=N, **kw)


def _forcing(model, target):
    """One table row per cell of every target map, allowing exactly target[b, f, t]: (table [B F T, n], map [B, F, T])."""
    B, F, T = target.shape
    n = model.n_class_target
    table = torch.full((B * F * T, n), -float("inf"))
    table[torch.arange(B * F * T), target.reshape(-1)] = 0.0
    return table, torch.arange(B * F * T).reshape(B, F, T)


def _windows(model):
    F, T = model.shape
    return [_window_mask(F, T, slice(0, F), slice(1, 3) if T == 4 else slice(3, 6)),
            _window_mask(F, T, slice(2, F - 1), slice(2, 4)), _window_mask(F, T, slice(0, F), slice(0, T))]


def _check_forced(name, got, init, target, mask):
    got, m = got.cpu(), mask.expand(got.shape[0], -1, -1)
    want = torch.where(m, target.expand_as(got), init.expand_as(got))
    wrong = (got != want)
    assert not bool(wrong.any()), (f"{name}: {int((wrong & m).sum())} sampled cells are not their target, "
                                   f"{int((wrong & ~m).sum())} cells outside the window changed; first {wrong.nonzero()[:4].tolist()}")


@pytest.mark.parametrize("graph", [0, 1, 3, None])
def test_loop_reads_each_cells_bias_row(golden_dir, graph):
    """A table with one row per cell, each allowing exactly target[f, t] of a random target map, given as code_bias_map over
    a window: the sampled window equals the target exactly and nothing outside it changes, whatever the uniforms -- on the
    golden top (time-major order) and bottom (zig-zag order) priors, B = 1 with a [F, T] map and B = 3 with a per-row
    [B, F, T] map of different targets, windows and the whole map, fp32 and bf16 caches, direct launches
    (ISI_PRIOR_GRAPH = 0) and graphs of 1, 3 and the default 8 positions.  Any error in sequence order, per-row stride,
    position offset or the replayed position counter draws a class the target row bans."""
    from interactive_spectrogram_inpainting import _hip
    _, top, bottom = _models(golden_dir)
    ctx = _hip.knob("ISI_PRIOR_GRAPH", graph) if graph is not None else contextlib.nullcontext()
    with ctx:
        for model, name, seed in ((top, "top", 401), (bottom, "bottom", 402)):
            S = model.target_transformer_sequence_length
            for wi, mask in enumerate(_windows(model)):
                for B, kv in ((1, None), (3, None), (3, torch.bfloat16)):
                    init, cond, g = _request(model, seed + 10 * wi + B, B)
                    target = torch.randint(0, 32, init.shape, generator=g)
                    table, cells = _forcing(model, target)
                    uni = torch.rand(S, B, generator=g)
                    got = _sample(model, B, uni, init, cond, mask, kv=kv, code_bias=table,
                                  code_bias_map=cells[0] if B == 1 else cells)
                    _check_forced(f"{name} window {wi} B={B} kv={kv} graph={graph}", got, init, target, mask)


@pytest.mark.parametrize("graph", [0, None])
def test_ragged_loop_reads_each_rows_bias_row(golden_dir, graph):
    """Two requests with different windows and different targets in one ragged call (isi_prior_sample_run_rows: every row
    at its own position, the index read by the row's own token)."""
    from interactive_spectrogram_inpainting import _hip
    _, top, bottom = _models(golden_dir)
    ctx = _hip.knob("ISI_PRIOR_GRAPH", graph) if graph is not None else contextlib.nullcontext()
    with ctx:
        for model, name, seed in ((top, "top", 411), (bottom, "bottom", 412)):
            w = _windows(model)
            for mask, kv in ((torch.cat([w[0], w[1]]), None), (torch.cat([w[1], w[2]]), torch.bfloat16)):
                init, cond, g = _request(model, seed, 2)
                target = torch.randint(0, 32, init.shape, generator=g)
                table, cells = _forcing(model, target)
                uni = torch.rand(model.target_transformer_sequence_length, 2, generator=g)
                got = _sample(model, 2, uni, init, cond, mask, kv=kv, temperature=[0.7, 1.1], code_bias=table, code_bias_map=cells)
                _check_forced(f"ragged {name} kv={kv} graph={graph}", got, init, target, mask)


@pytest.mark.parametrize("N", [3, 48])
def test_variations_read_each_cells_bias_row(golden_dir, N):
    """num_variations at 3 rows and at 48 (the row-block cross-attention over the shared memory): one request, one [F, T]
    map, every variation is forced to the target."""
    from interactive_spectrogram_inpainting import _hip
    _, top, bottom = _models(golden_dir)
    for graph in (0, None):
        ctx = _hip.knob("ISI_PRIOR_GRAPH", graph) if graph is not None else contextlib.nullcontext()
        with ctx:
            for model, name, seed in ((top, "top", 421), (bottom, "bottom", 422)):
                mask = _windows(model)[0]
                init, cond, g = _request(model, seed)
                target = torch.randint(0, 32, init.shape, generator=g)
                table, cells = _forcing(model, target)
                uni = torch.rand(model.target_transformer_sequence_length, N, generator=g)
                got = _sample(model, 1, uni, init, cond, mask, N=N, code_bias=table, code_bias_map=cells[0])
                assert got.shape[0] == N
                _check_forced(f"variations {name} N={N} graph={graph}", got, init, target, mask)


def _palettes(model, g):
    """Two disjoint palettes of 12 and 10 classes as a table [2, n], and the sets."""
    n = model.n_class_target
    perm = torch.randperm(32, generator=g)
    sets = (perm[:12], perm[12:22])
    table = torch.full((2, n), -float("inf"))
    for r, s in enumerate(sets):
        table[r, s] = 0.0
    return table, sets


def test_palettes_per_region_and_allowed_codes(golden_dir):
    """Two disjoint palettes over the two halves of a window: every sampled code lies in its cell's palette; allowed_codes
    over the whole map does the same; a zero code_bias gives the codes of the call without the option."""
    _, top, bottom = _models(golden_dir)
    for model, name, seed in ((top, "top", 431), (bottom, "bottom", 432)):
        F, T = model.shape
        S = model.target_transformer_sequence_length
        mask = _window_mask(F, T, slice(0, F), slice(0, T))
        init, cond, g = _request(model, seed, 2)
        table, sets = _palettes(model, g)
        cells = torch.full((F, T), -1, dtype=torch.int64)
        cells[:F // 2], cells[F // 2:] = 0, 1
        uni = torch.rand(S, 2, generator=g)
        got = _sample(model, 2, uni, init, cond, mask, temperature=1.0, top_k=0, top_p=0.0, code_bias=table, code_bias_map=cells).cpu()
        for r, rows in enumerate((got[:, :F // 2], got[:, F // 2:])):
            assert bool(torch.isin(rows, sets[r]).all()), f"{name}: a code outside palette {r}"
            assert len(rows.unique()) > 3, f"{name}: palette {r} is hardly used"
        allowed = torch.zeros(model.n_class_target, dtype=torch.bool)
        allowed[sets[0]] = True
        for given in (allowed, sets[0].tolist()):
            got = _sample(model, 2, uni, init, cond, mask, temperature=1.0, top_k=0, top_p=0.0, allowed_codes=given).cpu()
            assert bool(torch.isin(got, sets[0]).all()), f"{name}: allowed_codes let another class through"
        window = _windows(model)[0]
        plain = _sample(model, 2, uni, init, cond, window)
        assert not bool(torch.isin(plain.cpu()[window.expand(2, -1, -1)], sets[0]).all())     # (the palette does restrict)
        for kw in (dict(code_bias=torch.zeros(model.n_class_target)),
                   dict(code_bias=torch.zeros(3, model.n_class_target), code_bias_map=cells + 1),
                   dict(code_bias=table, code_bias_map=torch.full((2, F, T), -1))):
            assert torch.equal(_sample(model, 2, uni, init, cond, window, **kw), plain), f"{name}: {sorted(kw)} moved the codes"


def test_ragged_batch_of_biased_requests_equals_single_calls(golden_dir):
    """Two requests with different windows, one with a palette and one with a dense bias, in one ragged call == the two
    single calls (tests/test_batched_inpainting_gpu.py does this for masks)."""
    _, top, bottom = _models(golden_dir)
    for model, name, seed in ((top, "top", 441), (bottom, "bottom", 442)):
        F, T = model.shape
        w = _windows(model)
        mask = torch.cat([w[0], w[1]])
        init, cond, g = _request(model, seed, 2)
        table, _ = _palettes(model, g)
        table[1] = torch.randn(model.n_class_target, generator=g) * 3.0
        cells = torch.stack([torch.zeros(F, T, dtype=torch.int64), torch.ones(F, T, dtype=torch.int64)])
        uni = torch.rand(model.target_transformer_sequence_length, 2, generator=g)
        both = _sample(model, 2, uni, init, cond, mask, code_bias=table, code_bias_map=cells)
        unbiased = _sample(model, 2, uni, init, cond, mask)
        for r in range(2):
            alone = _sample(model, 1, uni[:, r:r + 1], init[r:r + 1], None if cond is None else cond[r:r + 1], mask[r:r + 1],
                            code_bias=table[r])
            assert torch.equal(both[r:r + 1], alone), f"{name}: request {r} samples other codes in the batch than alone"
            assert not torch.equal(both[r], unbiased[r]), f"{name}: request {r}: the bias changed nothing"


def test_variations_with_a_palette_equal_a_batch_of_repeated_inputs(golden_dir):
    _, top, bottom = _models(golden_dir)
    N = 4
    for model, name, seed in ((top, "top", 451), (bottom, "bottom", 452)):
        mask = _windows(model)[0]
        init, cond, g = _request(model, seed)
        table, _ = _palettes(model, g)
        uni = torch.rand(model.target_transformer_sequence_length, N, generator=g)
        var = _sample(model, 1, uni, init, cond, mask, N=N, allowed_codes=torch.isfinite(table[0]))
        rep = _sample(model, N, uni, init.repeat(N, 1, 1), None if cond is None else cond.repeat(N, 1, 1), mask,
                      allowed_codes=torch.isfinite(table[0]))
        assert torch.equal(var, rep), f"{name}: num_variations with a palette differs from the batch of repeated inputs"


def test_log_probs_stay_the_models(golden_dir):
    """return_log_probs with a bias: the values equal score_codemap of the result at LOOP_TOL -- the model's
    log-probability, not the biased distribution's (under a palette of 12 of 33 classes the two differ by nats)."""
    import sample as S
    _, top, bottom = _models(golden_dir)
    for model, name, seed in ((top, "top", 461), (bottom, "bottom", 462)):
        mask = _windows(model)[0]
        init, cond, g = _request(model, seed, 2)
        table, _ = _palettes(model, g)
        uni = torch.rand(model.target_transformer_sequence_length, 2, generator=g)
        codes, lp = _sample(model, 2, uni, init, cond, mask, allowed_codes=torch.isfinite(table[0]), return_log_probs=True)
        assert torch.equal(codes, _sample(model, 2, uni, init, cond, mask, allowed_codes=torch.isfinite(table[0])))
        tf = S.score_codemap(model, _dev(), codes, condition=(init if model.self_conditional_model else cond),
                             class_conditioning=CLS, mask=mask)
        m = mask.expand(2, -1, -1).to(lp.device)
        assert bool((lp[~m] == 0.0).all()) and bool((lp[m] < 0.0).all())
        print(f"log-probs under a palette, {name}: max |in-loop - teacher-forced| = {float((lp - tf).abs().max()):.3e}")
        _close(lp, tf, LOOP_TOL, f"{name}: in-loop vs teacher-forced under a palette")


# ---------------------------------------------------------------- inpainting

def _sound(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 32, (1, 8, 10), generator=g).to(dev), torch.randint(0, 32, (1, 16, 20), generator=g).to(dev)


def test_timerange_change_with_another_sounds_palette(golden_dir):
    """allowed_codes_top = codes_in_use(another top map): the window's new top codes lie in the set, nothing outside the
    window changes; the bottom stage of the same request takes its own palette."""
    import inpainting as I
    import sample as S
    _, top, bottom = _models(golden_dir)
    dev = _dev()
    top_code, bottom_code = _sound(dev, 7)
    other_top = torch.randint(0, 9, (1, 8, 10), generator=torch.Generator().manual_seed(8))
    other_bottom = torch.randint(20, 31, (1, 16, 20), generator=torch.Generator().manual_seed(9))
    used_t, used_b = S.codes_in_use(other_top, top.n_class_target), S.codes_in_use(other_bottom, bottom.n_class_target)
    mask = _window_mask(8, 4, slice(1, 7), slice(1, 3))
    for extra in ({}, {"num_variations": 3}):
        new_top, new_bottom = I.timerange_change(top, bottom, top_code, bottom_code, mask, "top", 3, 0.9, CLS, CLS, dev,
                                                 generator=torch.Generator().manual_seed(1), allowed_codes_top=used_t,
                                                 allowed_codes_bottom=used_b, **extra)
        full = torch.zeros(1, 8, 10, dtype=torch.bool)
        full[..., 3:7] = mask
        full_b = torch.zeros(1, 16, 20, dtype=torch.bool)
        full_b[..., 6:14] = mask.repeat_interleave(2, -2).repeat_interleave(2, -1)
        for new, old, m, used in ((new_top, top_code, full, used_t), (new_bottom, bottom_code, full_b, used_b)):
            new, m = new.cpu(), m.expand(new.shape[0], -1, -1)
            assert bool(used[new[m]].all()), "a new code outside the other sound's palette"
            assert torch.equal(new[~m], old.cpu().expand_as(new)[~m]), "a code outside the window changed"
        assert not bool(used_t[top_code.cpu()[full]].all())                  # (the old window was not in the palette)


def test_timerange_change_batch_with_biased_and_unbiased_requests(golden_dir):
    """One biased and one unbiased request per layer in one batch == the single calls with equally seeded generators."""
    import inpainting as I
    _, top, bottom = _models(golden_dir)
    dev = _dev()
    top_code, bottom_code = _sound(dev, 17)
    g = torch.Generator().manual_seed(18)
    pal_t, _ = _palettes(top, g)
    pal_b, _ = _palettes(bottom, g)
    cells_b = torch.zeros(16, 8, dtype=torch.int64)
    cells_b[:, 4:] = 1
    specs = [("top", 0, _window_mask(8, 4, slice(0, 8), slice(1, 3)), dict(allowed_codes_top=torch.isfinite(pal_t[0]),
                                                                           code_bias_bottom=pal_b, code_bias_map_bottom=cells_b)),
             ("top", 6, _window_mask(8, 4, slice(2, 5), slice(0, 4)), dict(top_k_sampling_k=4)),
             ("bottom", 5, _window_mask(16, 8, slice(3, 12), slice(2, 5)), dict(code_bias_bottom=pal_b[0].clone())),
             ("bottom", 2, _window_mask(16, 8, slice(0, 16), slice(6, 8)), {}),
             ("bottom", 1, _window_mask(16, 8, slice(0, 16), slice(3, 5)), dict(allowed_codes_bottom=torch.isfinite(pal_b[1])))]
    requests, expected = [], []
    for i, (layer, start, m, extra) in enumerate(specs):
        base = dict(top_code=top_code, bottom_code=bottom_code, mask=m, layer=layer, start_index_top=start,
                    temperature=0.8 + 0.05 * i, class_conditioning_top=CLS, class_conditioning_bottom=CLS, **extra)
        requests.append(dict(base, generator=torch.Generator().manual_seed(70 + i)))
        expected.append(I.timerange_change(top, bottom, device=dev, generator=torch.Generator().manual_seed(70 + i), **base))
    got = I.timerange_change_batch(top, bottom, requests, dev)
    for i, ((t, b), (te, be)) in enumerate(zip(got, expected)):
        assert torch.equal(t, te), f"request {i}: top map"
        assert torch.equal(b, be), f"request {i}: bottom map"
    plain = I.timerange_change_batch(top, bottom, [dict({k: v for k, v in q.items() if k not in I._CODE_BIAS_KEYWORDS},
                                                        generator=torch.Generator().manual_seed(70 + i))
                                                   for i, q in enumerate(requests)], dev)
    assert not torch.equal(plain[0][0], got[0][0]), "the palette changed nothing"
