"""The categorical draw kernel (sample_row_f32_kernel: temperature, top-k, top-p, inverse-CDF draw) against the float64
specification of tests/tests_support.py, at the real sizes: 512 / 513 classes (16 waves, the cross-wave stages of the sort
and of the prefix sums) and the shapes around every wave and workgroup edge.  The filter must equal the specification's
exactly; every draw must pass the one acceptance rule of `tests_support.sampling_accepts`.  Both entries are driven:
`_ops.sample_rows` (the plain instantiation) and `_ops.sample_rows_log_probs` (the one with log-probabilities).
tests/test_sampling_spec_host.py shows, without a GPU, that the rows and filters used here leave no cut ambiguous."""
import time

import numpy as np
import pytest
import torch

import tests_support as TS
from test_prior_gpu import _dev

pytestmark = pytest.mark.gpu

CHUNK = 65536                                            # rows per launch, at most
# the 128 largest floats below 1: with classes of zero probability behind the last non-zero one (top_k = 40 of 512, the
# masked 513th class) this is where a prefix that stays <= u * total sends the draw to the kernel's fallback class
TOP_ULPS = (np.float32(1.0).view(np.int32) - np.arange(128, 0, -1, dtype=np.int32)).view(np.float32)
# a recording aid, not a check: figures of the tests that ran in this process, printed by each of them as it ends
STATS = {"t0": None, "rows": 0, "differ": 0, "tiny": 0, "min_rel": float("inf"), "max_rel": 0.0}


def _device_rows(c, rows, dev):
    """[rows, n] view of a [rows, stride] buffer, the case's logits in every row and NaN behind them."""
    buf = torch.full((rows, c.stride), float("nan"), dtype=torch.float32, device=dev)
    view = buf[:, :c.logits.shape[0]]
    view.copy_(torch.from_numpy(c.logits).to(dev).expand_as(view))
    return view


def _draw_all(c, u, dev, log_probs):
    """Tokens of sample_rows for every uniform (logits repeated per row, launches of at most CHUNK rows); with log_probs
    also the tokens and values of sample_rows_log_probs and token_log_probs of those tokens."""
    from interactive_spectrogram_inpainting.priors import _ops
    tok, tok2, lp, lp2 = [], [], [], []
    for i in range(0, u.shape[0], CHUNK):
        uc = torch.from_numpy(u[i:i + CHUNK]).to(dev)
        view = _device_rows(c, uc.shape[0], dev)
        tok.append(_ops.sample_rows(view, c.temperature, c.top_k, c.top_p, uc))
        if log_probs:
            t2, l2 = _ops.sample_rows_log_probs(view, c.temperature, c.top_k, c.top_p, uc)
            tok2.append(t2)
            lp.append(l2)
            lp2.append(_ops.token_log_probs(view, t2))
    cat = lambda v: torch.cat(v).cpu().numpy()
    return (cat(tok), cat(tok2), cat(lp), cat(lp2)) if log_probs else cat(tok)


@pytest.fixture(autouse=True)
def _clock():
    if STATS["t0"] is None:
        STATS["t0"] = time.perf_counter()


def _record(spec, u, tok):
    """Where the kernel's draw differs from the float64 draw: the relative distance of u from the boundary between them."""
    STATS["rows"] += int(u.shape[0])
    ref = TS.sampling_float64_draw(spec, u)
    d = np.flatnonzero(tok != ref)
    if not d.shape[0]:
        return
    u64 = u.astype(np.float64)[d]
    lower = np.concatenate([[0.0], spec.cdf])[ref[d]]    # the edges of the float64 draw's interval
    upper = spec.cdf[ref[d]]
    dist = np.abs(u64 - np.where(tok[d] < ref[d], lower, upper))
    STATS["differ"] += int(d.shape[0])
    big = dist > spec.cdf.shape[0] * 2.0 ** -126         # (the others: classes under fp32 resolution skipped at u = 0)
    STATS["tiny"] += int((~big).sum())
    if not big.any():
        return
    rel = dist[big] / u64[big]
    STATS["min_rel"] = min(STATS["min_rel"], float(rel.min()))
    STATS["max_rel"] = max(STATS["max_rel"], float(rel.max()))


def _report(what):
    m = f"{STATS['min_rel']:.3e} .. {STATS['max_rel']:.3e}" if STATS["differ"] > STATS["tiny"] else "none"
    m += f", {STATS['tiny']} more within n 2^-126 of it"
    print(f"{what}: {STATS['rows']} rows checked so far; kernel draw != float64 draw on {STATS['differ']} of them, "
          f"relative |u - boundary| there: {m} (tau = {TS.SAMPLING_TAU:.3e}); {time.perf_counter() - STATS['t0']:.1f} s "
          "since the first test of this file began")


@pytest.mark.parametrize("n", TS.SAMPLING_SHAPES)
def test_filter_equals_float64_spec_exactly(n):
    """isfinite(filtered) == the specification's kept mask, no class excused; kept values == float32(logits) *
    float32(1 / T) bit for bit and removed ones are -inf; on every (row, filter) case of the shape, row stride n or n + 5
    with NaN behind the row.  MI355X: every case of every shape passes (1957 cases)."""
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    bad = []
    cases = TS.sampling_cases(n)
    for c in cases:
        spec = TS.sampling_spec(c.logits, c.temperature, c.top_k, c.top_p)
        _, filt = _ops.sample_rows(_device_rows(c, 2, dev), c.temperature, c.top_k, c.top_p, torch.tensor([0.25, 0.75]),
                                   return_filtered=True)
        filt = filt.cpu().numpy()
        want = np.where(spec.kept, spec.lg, np.float32(-np.inf)).astype(np.float32)
        for r in range(2):
            if not np.array_equal(np.isfinite(filt[r]), spec.kept):
                wrong = np.flatnonzero(np.isfinite(filt[r]) != spec.kept)
                bad.append(f"{c.name} T={c.temperature} k={c.top_k} p={c.top_p!r}: kept mask differs at classes "
                           f"{wrong[:8].tolist()} ({wrong.shape[0]} in all)")
            elif not np.array_equal(filt[r].view(np.int32), want.view(np.int32)):
                bad.append(f"{c.name}: kept values are not float32(logits) * float32(1 / T) bit for bit")
    print(f"n={n}: {len(cases)} filter cases, {len(bad)} wrong")
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("n", TS.SAMPLING_SHAPES)
def test_draws_pass_the_acceptance_rule(n):
    """Per (row, filter) case of the shape, the uniforms (a) at the float64 midpoint of every kept class's interval -- a
    class whose interval is wider than 4 tau must come back exactly --, (b) 0 and the 128 largest floats below 1, (c) the boundary
    sweep: around float32(boundary) of every CDF boundary next to a zero-probability class (removed by top-k / top-p or
    masked by the caller) and 16 of the others, every float32 within 128 ulps.  Every draw must be a kept class of non-zero
    probability whose interval meets [u (1 - tau), u (1 + tau)]; on the sweep it must be one of the two non-zero classes at
    the boundary wherever both are wider than 4 tau.  sample_rows_log_probs must draw the same tokens and its
    log-probability must equal token_log_probs of the token bit for bit.

    MI355X, an earlier revision of this file with one uniform below 1 per case where there are now 128
    (profiles/sampling_draw_checks.txt): 6 795 349 rows over the ten shapes, 7 586 585 with the grids and the equal
    rows.  The kernel's draw differed from the float64 draw on 48 530 of them, the nearest at a relative |u - boundary| of
    1.0e-11; no draw of the corrected kernel was a removed or masked class.  The kernel before the correction drew such a
    class on the sweep at every shape from 63 classes up (top_k = 40, top_p ~ 0.8), one to nine uniforms per case."""
    dev = _dev()
    tau = TS.SAMPLING_TAU
    bad = []
    for c in TS.sampling_cases(n):
        spec = TS.sampling_spec(c.logits, c.temperature, c.top_k, c.top_p)
        nz = np.flatnonzero(spec.kept & (spec.prob > 0.0))
        lower = np.concatenate([[0.0], spec.cdf])[nz]
        width = spec.cdf[nz] - lower
        u_mid = (lower + 0.5 * width).astype(np.float32)
        u_mid = np.minimum(u_mid, np.nextafter(np.float32(1.0), np.float32(0.0)))
        u_end = np.concatenate([np.zeros(1, dtype=np.float32), TOP_ULPS])
        u_sw, b_sw = TS.sampling_sweep_uniforms(spec)
        u = np.concatenate([u_mid, u_end, u_sw])
        tok, tok2, lp, lp2 = _draw_all(c, u, dev, log_probs=True)
        _record(spec, u, tok)
        tag = f"{c.name} T={c.temperature} k={c.top_k} p={c.top_p!r}"
        ok, first, last = TS.sampling_accepts(spec, u, tok)
        for i in np.flatnonzero(~ok)[:4]:
            kind = "midpoint" if i < u_mid.shape[0] else "end" if i < u_mid.shape[0] + u_end.shape[0] else "sweep"
            state = "kept" if spec.kept[tok[i]] else "NOT KEPT"
            bad.append(f"{tag}: {kind} u={u[i]!r} drew class {tok[i]} ({state}, probability {spec.prob[tok[i]]:.3e}); "
                       f"accepted: non-zero classes {first[i]} .. {last[i]} ({int((~ok).sum())} such draws in this case)")
        wide = width > 4 * tau                            # (a) exact where the interval is wide
        exact = tok[:u_mid.shape[0]] == nz
        assert (first[:u_mid.shape[0]][wide] == last[:u_mid.shape[0]][wide]).all(), "the rule itself must be decisive here"
        if not exact[wide].all():
            bad.append(f"{tag}: midpoint of a wide class drew another class, classes {nz[wide & ~exact][:8].tolist()}")
        if u_sw.shape[0]:                                 # (c) next to the boundary
            t_sw = tok[u_mid.shape[0] + u_end.shape[0]:]
            both_wide = wide[b_sw] & wide[b_sw + 1]
            beside = (t_sw == nz[b_sw]) | (t_sw == nz[b_sw + 1])
            if not beside[both_wide].all():
                i = np.flatnonzero(both_wide & ~beside)
                bad.append(f"{tag}: sweep drew a class that is not at the boundary, e.g. u={u_sw[i[0]]!r} class {t_sw[i[0]]} "
                           f"for the boundary between {nz[b_sw[i[0]]]} and {nz[b_sw[i[0]] + 1]} ({i.shape[0]} such draws)")
        if not np.array_equal(tok, tok2):
            bad.append(f"{tag}: sample_rows_log_probs drew other tokens than sample_rows on {int((tok != tok2).sum())} rows")
        if not np.array_equal(lp.view(np.int32), lp2.view(np.int32)):
            bad.append(f"{tag}: the draw's log-probability differs from token_log_probs of its token")
    _report(f"n={n}")
    assert not bad, f"{len(bad)} findings, the first:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("row", range(3))
def test_stratified_grid_passes_the_acceptance_rule(row):
    """u = (j + 0.5) / 2^18, j = 0 .. 2^18 - 1, on a 512-class row, a 513-class row and a 513-class row with the mask token
    excluded and top_k = 40: every draw passes the acceptance rule, which bounds every class's count by its probability
    (no statistical threshold).  MI355X (this test is unchanged since that run): 3 x 262 144 draws, all accepted,
    before and after the kernel's correction."""
    dev = _dev()
    name, logits, t, k, p = TS.sampling_grid_rows()[row]
    c = TS.SamplingCase(name, logits, t, k, p, logits.shape[0] + (3 if row == 1 else 0))
    spec = TS.sampling_spec(logits, t, k, p)
    u = TS.sampling_grid_uniforms()
    tok = _draw_all(c, u, dev, log_probs=False)
    _record(spec, u, tok)
    ok, first, last = TS.sampling_accepts(spec, u, tok)
    ref = TS.sampling_float64_draw(spec, u)
    counts = np.bincount(tok, minlength=logits.shape[0])
    print(f"grid {name}: {u.shape[0]} draws, {int((tok != ref).sum())} differ from the float64 draw, "
          f"{int((first != last).sum())} uniforms accept more than one class, "
          f"largest |count - 2^18 p| = {np.abs(counts - 2.0 ** 18 * spec.prob).max():.2f}")
    _report(f"grid {name}")
    assert not counts[~spec.kept].any(), f"{name}: drew classes outside the kept set: {np.flatnonzero(counts * ~spec.kept)}"
    assert ok.all(), f"{name}: {int((~ok).sum())} draws refused, e.g. u={u[~ok][0]!r} class {tok[~ok][0]}"


@pytest.mark.parametrize("n,masked", [(2, False), (64, False), (64, True), (512, False), (512, True), (1024, False),
                                      (1024, True)])
def test_exact_boundaries_on_equal_logits(n, masked):
    """Where fp32 is exact there is no tolerance: on a row of equal logits (every second class masked with -inf when
    `masked`) every term is expf(0) = 1, every prefix an integer and the total a power of two, so for u = j / kept the
    product u * total is the integer j and the draw is decided by the comparison alone: `inc > u * total` gives the j-th
    kept class, as the float64 draw does; `>=` would give the one before."""
    dev = _dev()
    logits = np.full(n, 3.5, dtype=np.float32)
    if masked:
        logits[1::2] = -np.inf
    kept = n // 2 if masked else n
    u = (np.arange(kept, dtype=np.float64) / kept).astype(np.float32)
    for t, k in ((1.0, 0), (0.7, n)):
        c = TS.SamplingCase("equal", logits, t, k, 0.0, n + 1)
        spec = TS.sampling_spec(logits, t, k, 0.0)
        assert np.array_equal(spec.cdf[spec.kept], np.arange(1, kept + 1) / kept)
        tok, tok2, lp, lp2 = _draw_all(c, u, dev, log_probs=True)
        STATS["rows"] += int(u.shape[0])
        assert np.array_equal(tok, TS.sampling_float64_draw(spec, u)), (t, k, np.flatnonzero(tok != TS.sampling_float64_draw(spec, u))[:8])
        assert np.array_equal(tok, tok2) and np.array_equal(lp.view(np.int32), lp2.view(np.int32))
        _report(f"equal logits n={n} masked={masked}")
