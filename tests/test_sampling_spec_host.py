"""The float64 specification of the categorical draw (tests/tests_support.py) on its own, without a GPU: it agrees with
oracle/prior_oracle.py where the oracle is well defined, and the rows, filters and uniforms that
tests/test_sampling_draw_gpu.py sends to the kernel satisfy the conditions its exact comparisons rely on."""
import numpy as np
import pytest
import torch

import tests_support as TS
from oracle import prior_oracle as P


def _oracle_kept(lg, top_k, top_p):
    return torch.isfinite(P.top_k_top_p_filtering(torch.from_numpy(lg).double(), top_k, top_p)).numpy()


def test_reciprocal_temperature_is_unambiguous():
    for t in TS.SAMPLING_TEMPERATURES:
        assert np.float32(1.0) / np.float32(t) == np.float32(1.0 / t), t


def test_filter_equals_oracle_on_the_golden_rows(golden_dir):
    z = np.load(golden_dir / "filtering.npz")
    logits = z["logits"].reshape(-1, z["logits"].shape[-1])
    for key in z.files:
        if key == "logits":
            continue
        k, p = key[1:].split("_p")
        want = np.isfinite(z[key]).reshape(logits.shape)
        for r, row in enumerate(logits):
            spec = TS.sampling_spec(row, 1.0, int(k), float(p))
            assert np.array_equal(spec.kept, want[r]), (key, r)
            assert np.array_equal(spec.lg, row)


@pytest.mark.parametrize("n", TS.SAMPLING_SHAPES)
def test_filter_equals_oracle_on_tie_free_rows(n):
    """On rows without equal logits the oracle's torch.sort is well defined; the oracle runs in float64 on the same lg."""
    checked = 0
    for c in TS.sampling_cases(n):
        lg = TS.sampling_scaled_logits(c.logits, c.temperature)
        fin = lg[np.isfinite(lg)]
        if np.unique(fin).shape[0] != fin.shape[0]:
            continue
        spec = TS.sampling_spec(c.logits, c.temperature, c.top_k, c.top_p)
        assert np.array_equal(spec.kept, _oracle_kept(lg, c.top_k, c.top_p)), c.name
        checked += 1
    assert checked >= 100


@pytest.mark.parametrize("n", [2, 65, 512, 513, 1024])
def test_draw_equals_oracle_away_from_boundaries(n):
    g = np.random.default_rng(n)
    for c in TS.sampling_cases(n)[::7]:
        spec = TS.sampling_spec(c.logits, c.temperature, c.top_k, c.top_p)
        u = g.random(2000).astype(np.float32)
        d = np.abs(u.astype(np.float64)[:, None] - spec.cdf[None, :]).min(1)
        u = u[d > 1e-6]
        ref = P.sample_from_uniform(torch.from_numpy(spec.prob), torch.from_numpy(u).double()).numpy()
        assert np.array_equal(TS.sampling_float64_draw(spec, u), ref), c.name
        ok, first, last = TS.sampling_accepts(spec, u, ref)
        assert ok.all(), c.name


@pytest.mark.parametrize("n", TS.SAMPLING_SHAPES)
def test_cases_meet_the_conditions_of_the_gpu_tests(n):
    """Every top_p lies SAMPLING_TOP_P_MARGIN or more from every deciding cumulative of its row (after the float32 cast), so
    no cut is ambiguous in fp32; every row has finite total mass; the rows are what their names claim; the case list
    covers the filters."""
    cases = TS.sampling_cases(n)
    seen = set()
    for c in cases:
        lg = TS.sampling_scaled_logits(c.logits, c.temperature).astype(np.float64)
        assert np.isfinite(lg).any() and not np.isnan(lg).any() and not np.isposinf(lg).any(), c.name
        assert np.isfinite(np.exp(lg - lg[np.isfinite(lg)].max()).sum()), c.name
        if c.top_p > 0.0:
            assert np.float32(c.top_p) == c.top_p, c.name
            cum = TS.sampling_top_p_cumulatives(c.logits, c.temperature, c.top_k)
            if cum.shape[0]:
                assert np.abs(cum - c.top_p).min() >= TS.SAMPLING_TOP_P_MARGIN, c.name
        spec = TS.sampling_spec(c.logits, c.temperature, c.top_k, c.top_p)
        assert spec.kept.any() and np.isfinite(spec.cdf).all() and spec.cdf[-1] == 1.0, c.name
        row, k, p = c.name.split("/")
        seen.add((k, p))
        if p == "pone":
            assert spec.kept.sum() == 1, c.name
        if p == "ptie":                          # the cut parts equal logits: the lower indices stay
            cut = c.logits == c.logits[spec.kept].min()
            assert cut.sum() >= 3 and np.array_equal(np.flatnonzero(cut)[:2], np.flatnonzero(cut & spec.kept)), c.name
        if row.startswith("ties_k") and c.top_k in (5, 40) and n >= c.top_k + 4 and c.top_p == 0.0:
            assert spec.kept.sum() > c.top_k, c.name
        if row == "masked" and n >= 2:
            assert np.isinf(c.logits).sum() == len(range(1, n, 3)) and not spec.kept[1::3].any()
    if n >= 63:
        assert seen == {(f"k{k}", f"p{p}") for k, p in TS.SAMPLING_FILTERS}, seen
    assert {c.stride for c in cases} == {n, n + 5}


def test_top_p_one_is_exercised_at_the_real_sizes():
    for n in (512, 513):
        assert sum(c.top_p == 1.0 for c in TS.sampling_cases(n)) >= 10


@pytest.mark.parametrize("n", [512, 513, 1024])
def test_sweep_uniforms_walk_single_ulps(n):
    for c in TS.sampling_cases(n)[::11]:
        spec = TS.sampling_spec(c.logits, c.temperature, c.top_k, c.top_p)
        u, b = TS.sampling_sweep_uniforms(spec)
        if not u.shape[0]:
            continue
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
        nz = np.flatnonzero(spec.kept & (spec.prob > 0))
        u0 = spec.cdf[nz[b]].astype(np.float32)
        assert (np.abs(u.view(np.int32).astype(np.int64) - u0.view(np.int32)) <= 128).all()
        first = np.flatnonzero(b == b[0])
        assert (np.diff(u[first].view(np.int32)) == 1).all()
        gaps = np.flatnonzero(np.diff(nz) > 1)
        assert np.isin(gaps, b).all(), "a boundary next to a zero-probability class is missing"


def test_stratified_grid_is_nearly_everywhere_decisive():
    """A condition, not a measurement: at most 2 % of the grid's uniforms may accept more than one class (expected: kept
    boundaries * 2 tau * mean u ~ 512 * 2^-17 = 0.4 % at 512 kept classes)."""
    u = TS.sampling_grid_uniforms()
    assert u.shape[0] == 2 ** 18 and np.array_equal(u.astype(np.float64), (np.arange(2 ** 18) + 0.5) / 2.0 ** 18)
    for name, logits, t, k, p in TS.sampling_grid_rows():
        spec = TS.sampling_spec(logits, t, k, p)
        ok, first, last = TS.sampling_accepts(spec, u, TS.sampling_float64_draw(spec, u))
        assert ok.all(), name
        share = float((first != last).mean())
        print(f"{name}: {int(spec.kept.sum())} kept classes, {share:.4%} of the grid accepts more than one class")
        assert share <= 0.02, (name, share)


def test_acceptance_rule_rejects_what_it_must():
    logits = np.array([0.0, -np.inf, 0.0, 1.0, -2000.0], dtype=np.float32)
    spec = TS.sampling_spec(logits, 1.0, 0, 0.0)
    assert spec.kept.tolist() == [True, False, True, True, True] and spec.prob[4] == 0.0
    b = spec.cdf[0]
    u = np.float32(b) * np.ones(5, dtype=np.float32)
    ok, first, last = TS.sampling_accepts(spec, u, np.array([0, 1, 2, 3, 4]))
    assert ok.tolist() == [True, False, True, False, False]     # the masked class and the far class are refused
    ok, _, _ = TS.sampling_accepts(spec, np.float32([0.0, 0.0, 0.99999994, 0.99999994]), np.array([0, 2, 3, 4]))
    assert ok.tolist() == [True, False, True, False]            # (class 4 is kept but has zero probability)
