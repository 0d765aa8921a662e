"""Host side of the row statistics (isi_token_stats_f32, inpainting.select_unlikely / resample_unlikely): a float64
specification of the kernel's five outputs, held here to independent formulas; the C entry is exported, bound and refuses bad
arguments before any launch; the selection rule of resample_unlikely as a pure function on tensors.  No GPU."""
import ctypes
import math

import pytest
import torch

from test_log_probs_host import _bottom, _top

ISI_E_INVALID = -1


def spec_token_stats(logits: torch.Tensor, codes, top_n: int):
    """Float64 specification of isi_token_stats_f32 on fp32 logits [R, n] (codes int64 [R] or None):
    (log_prob float64 [R], entropy float64 [R], rank int64 [R], top_codes int64 [R, top_n], top_log_probs float64 [R, top_n]).
    Written from the definitions, class by class -- no sort, no log_softmax: those are what the tests below hold it to."""
    x = logits.double()
    R, n = x.shape
    z = x - x.max(-1, keepdim=True).values
    e = torch.exp(z)                                                 # a -inf logit: exactly 0
    tot = e.sum(-1, keepdim=True)
    logp = z - torch.log(tot)
    p = e / tot
    entropy = -torch.where(p > 0, p * logp, torch.zeros_like(p)).sum(-1)
    log_prob = torch.full((R,), float("nan"), dtype=torch.float64)
    rank = torch.full((R,), -1, dtype=torch.int64)
    top_codes = torch.full((R, top_n), -1, dtype=torch.int64)
    top_log_probs = torch.full((R, top_n), float("-inf"), dtype=torch.float64)
    index = torch.arange(n)
    for r in range(R):
        ahead_of = lambda c: int(((x[r] > x[r, c]) | ((x[r] == x[r, c]) & (index < c))).sum())
        if codes is not None and 0 <= int(codes[r]) < n:
            c = int(codes[r])
            log_prob[r] = logp[r, c]
            rank[r] = ahead_of(c)
        if top_n:
            ahead = torch.tensor([ahead_of(c) for c in range(n)])   # a permutation of 0 .. n - 1: the class's place
            for c in range(n):
                if ahead[c] < top_n:
                    top_codes[r, ahead[c]] = c
                    top_log_probs[r, ahead[c]] = logp[r, c]
    return log_prob, entropy, rank, top_codes, top_log_probs


def tie_rows(n: int, g: torch.Generator):
    """Rows [R, n] with exact ties and a code per row: values from a set of three, a maximum repeated at several classes
    (the code on a later one), runs of equal logits, +0 beside -0, -inf entries (the code on a finite class, then on a -inf
    one), one finite logit among -inf, and an all-equal row."""
    rows, codes = [], []
    pick = lambda: int(torch.randint(0, n, (1,), generator=g))
    rows.append(torch.randint(0, 3, (n,), generator=g).float())
    codes.append(pick())
    r = torch.randn(n, generator=g)
    at = torch.randperm(n, generator=g)[:max(1, min(5, n // 2))].sort().values
    r[at] = float(r.max()) + 1.0
    rows.append(r)
    codes.append(int(at[-1]))
    r = torch.randn(n, generator=g)
    r[n // 4:n // 4 + max(1, n // 3)] = 0.25
    rows.append(r)
    codes.append(min(n - 1, n // 4 + max(1, n // 3) - 1))
    r = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    rows.append(r)
    codes.append(n - 1)
    r = torch.randn(n, generator=g)
    r[torch.rand(n, generator=g) < 0.5] = float("-inf")
    r[n // 2] = 0.5
    rows.append(r)
    codes.append(n // 2)
    rows.append(r.clone())
    r2 = rows[-1]
    r2[0] = r2[n - 1] = float("-inf")
    r2[n // 2] = 0.5
    codes.append(n - 1)
    r = torch.full((n,), float("-inf"))
    r[(2 * n) // 3] = -3.0
    rows.append(r)
    codes.append((2 * n) // 3)
    rows.append(torch.full((n,), 1.75))
    codes.append(pick())
    return torch.stack(rows), torch.tensor(codes, dtype=torch.int64)


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300])
def test_spec_against_independent_formulas(n):
    g = torch.Generator().manual_seed(40 + n)
    ties, tie_codes = tie_rows(n, g)
    plain = torch.randn(4, n, generator=g) * 4
    logits = torch.cat([ties, plain])
    codes = torch.cat([tie_codes, torch.randint(0, n, (4,), generator=g)])
    top_n = 16
    log_prob, entropy, rank, top_codes, top_log_probs = spec_token_stats(logits, codes, top_n)
    want_lp = torch.log_softmax(logits.double(), -1)
    assert torch.allclose(log_prob, want_lp.gather(1, codes[:, None])[:, 0], rtol=0, atol=1e-12, equal_nan=True)
    order = torch.sort(logits, dim=-1, descending=True, stable=True).indices
    k = min(n, top_n)
    assert torch.equal(top_codes[:, :k], order[:, :k])
    assert bool((top_codes[:, k:] == -1).all()) and bool((top_log_probs[:, k:] == float("-inf")).all())
    assert torch.allclose(top_log_probs[:, :k], want_lp.gather(1, order[:, :k]), rtol=0, atol=1e-12)
    place = torch.argsort(order, dim=-1)                            # class -> its position in the stable descending sort
    assert torch.equal(rank, place.gather(1, codes[:, None])[:, 0])
    if n >= 4:
        assert int(rank[1]) >= 1, "the repeated maximum is not repeated"
    # entropy: n equal logits -> ln n; one finite logit among -inf -> 0; never negative, never above ln n
    assert abs(float(entropy[7]) - math.log(n)) <= 1e-12
    assert float(entropy[6]) == 0.0
    assert bool((entropy >= 0).all()) and bool((entropy <= math.log(n) + 1e-12).all())
    ref_entropy = torch.distributions.Categorical(logits=logits[-4:].double()).entropy()
    assert torch.allclose(entropy[-4:], ref_entropy, rtol=0, atol=1e-12)


def test_spec_out_of_range_codes_and_no_codes():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(3, 9, generator=g)
    log_prob, entropy, rank, top_codes, _ = spec_token_stats(logits, torch.tensor([9, -1, 4]), 2)
    assert torch.isnan(log_prob[:2]).all() and rank.tolist()[:2] == [-1, -1] and int(rank[2]) >= 0
    none = spec_token_stats(logits, None, 2)
    assert torch.equal(none[1], entropy) and torch.equal(none[3], top_codes)


def test_token_stats_entry_is_exported_bound_and_checks_its_arguments():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    assert "isi_token_stats_f32" in _hip.SIGNATURES
    fn = lib.isi_token_stats_f32
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12
    buf = (ctypes.c_float * 64)()
    codes = (ctypes.c_int64 * 64)()
    p, c = ctypes.addressof(buf), ctypes.addressof(codes)
    # (host placeholders behind the pointers: every call below must return before any launch)
    #      logits stride rows n codes log_prob entropy rank top_n top_codes top_log_probs
    bad = [(None, 8, 2, 8, c, p, p, p, 2, c, p),                                     # null logits
           (p, 8, 0, 8, c, p, p, p, 2, c, p), (p, 8, -1, 8, c, p, p, p, 2, c, p),    # rows <= 0
           (p, 8, 2, 0, c, p, p, p, 2, c, p), (p, 8, 2, -3, c, p, p, p, 2, c, p),    # n <= 0
           (p, 7, 2, 8, c, p, p, p, 2, c, p), (p, 0, 2, 8, c, p, p, p, 2, c, p),     # stride < n
           (p, 8, 2, 8, c, p, p, p, -1, c, p), (p, 8, 2, 8, c, p, p, p, 17, c, p),   # top_n outside 0 .. 16
           (p, 8, 2, 8, None, p, p, None, 2, c, p),                                  # log_prob without codes
           (p, 8, 2, 8, None, None, p, p, 2, c, p)]                                  # rank without codes
    for args in bad:
        assert fn(*args, None) == ISI_E_INVALID, args
        assert b"token_stats" in lib.isi_last_error(), args


def test_python_wrappers_check_their_arguments_before_any_device_work():
    import sample as S
    from interactive_spectrogram_inpainting.priors import _ops
    with pytest.raises(ValueError, match="top_n"):
        S.codemap_statistics(_top(), "cpu", torch.zeros(1, 8, 4, dtype=torch.int64), top_n=17)
    with pytest.raises(ValueError, match="self-conditional"):
        S.codemap_statistics(_bottom(), "cpu", torch.zeros(1, 16, 8, dtype=torch.int64))
    with pytest.raises(Exception):                                   # logits on the host
        _ops.token_stats(torch.zeros(2, 8))
    assert _ops.TokenStats._fields == ("log_probs", "entropy", "rank", "top_codes", "top_log_probs")
    assert S.CodemapStatistics._fields == _ops.TokenStats._fields


# ---------------------------------------------------------------- the selection rule

def _select(*a, **k):
    import inpainting as I
    return I.select_unlikely(*a, **k)


@pytest.mark.parametrize("size,fraction,count", [(10, 0.5, 5), (10, 0.25, 3), (10, 0.01, 1), (10, 1.0, 10), (10, 0.0, 0),
                                                 (7, 0.5, 4), (7, 1 / 7, 1), (3, 0.34, 2), (1, 0.5, 1), (32, 0.1, 4),
                                                 (0, 0.5, 0)])
def test_fraction_selects_the_ceiling_of_the_share_lowest_first(size, fraction, count):
    g = torch.Generator().manual_seed(size)
    lp = -torch.rand(1, 8, 4, generator=g) * 9
    region = torch.zeros(32, dtype=torch.bool)
    region[torch.randperm(32, generator=g)[:size]] = True
    region = region.reshape(1, 8, 4)
    outside = lp.clone()
    outside[~region] = -100.0                                        # far lower, but not allowed to change
    sel = _select(outside, region, fraction=fraction)
    assert sel.dtype == torch.bool and sel.shape == region.shape
    assert int(sel.sum()) == count == math.ceil(fraction * size)
    assert not bool((sel & ~region).any()), "the selection left the region"
    if 0 < count < size:
        assert float(lp[sel].max()) <= float(lp[region & ~sel].min())
    if count == 0:
        assert not bool(sel.any())


def test_ties_go_in_the_order_of_the_flattened_tensor():
    lp = torch.tensor([[-2.0, -5.0, -5.0, -1.0, -5.0, -5.0, -7.0, -5.0]])
    region = torch.tensor([[True, False, True, True, True, True, True, True]])
    # -7 first, then the -5s at 2, 4, 5, 7 in that order (the -5 at 1 lies outside the region)
    for count, want in ((1, [6]), (2, [2, 6]), (3, [2, 4, 6]), (4, [2, 4, 5, 6]), (5, [2, 4, 5, 6, 7]), (6, [0, 2, 4, 5, 6, 7])):
        sel = _select(lp, region, fraction=count / 7)
        assert sel.nonzero()[:, 1].tolist() == want, (count, sel)


def test_threshold_selects_every_token_below_it():
    lp = torch.tensor([[[-0.1, -3.0], [-2.999, -8.0], [-3.0, -3.001]]])
    region = torch.tensor([[[True, True], [True, False], [True, True]]])
    sel = _select(lp, region, log_prob_below=-3.0)
    assert sel.tolist() == [[[False, False], [False, False], [False, True]]]        # strictly below, inside the region
    assert _select(lp, region, log_prob_below=0.0).tolist() == region.tolist()
    assert not bool(_select(lp, region, log_prob_below=-50.0).any())               # an empty selection
    assert not bool(_select(lp, torch.zeros_like(region), fraction=1.0).any())     # an empty region


def test_exactly_one_rule():
    lp, region = torch.zeros(1, 2, 2), torch.ones(1, 2, 2, dtype=torch.bool)
    with pytest.raises(ValueError):
        _select(lp, region)
    with pytest.raises(ValueError):
        _select(lp, region, fraction=0.5, log_prob_below=-1.0)
    with pytest.raises(ValueError):
        _select(lp, region, fraction=1.5)
    with pytest.raises(ValueError):
        _select(lp, region[:, :1], fraction=0.5)
    import inpainting as I
    top, bottom = _top(), _bottom()
    cls = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}
    args = (top, bottom, torch.zeros(1, 8, 4, dtype=torch.int64), torch.zeros(1, 16, 8, dtype=torch.int64),
            torch.ones(1, 8, 4, dtype=torch.bool), "top", 0, 1.0, cls, cls, "cpu")
    with pytest.raises(ValueError, match="exactly one"):                                 # ... before any device work
        I.resample_unlikely(*args)
    with pytest.raises(ValueError, match="exactly one"):
        I.resample_unlikely(*args, fraction=0.5, log_prob_below=-1.0)
    with pytest.raises(ValueError, match="return_scores"):
        I.resample_unlikely(*args, fraction=0.5, sort_by_likelihood=True)
    with pytest.raises(ValueError, match="uniform_sampling"):
        I.resample_unlikely(*args, fraction=0.5, return_scores=True, uniform_sampling=True)
    with pytest.raises(TypeError, match="top_p"):                                        # a misspelt keyword, whatever is selected
        I.resample_unlikely(*args, log_prob_below=-1e9, top_p=0.9)
    with pytest.raises(TypeError):
        I.resample_unlikely(*args, fraction=0.5, mask=args[4])


def test_keywords_resample_unlikely_accepts_are_timerange_changes():
    import inspect
    import inpainting as I
    import sample as S
    own = {"uniform_sampling", "generator", "kv_cache_dtype", "num_variations", "return_scores", "sort_by_likelihood"}
    assert own <= I._TIMERANGE_CHANGE_KEYWORDS
    assert {"top_k_sampling_k", "top_p_sampling_p"} <= I._TIMERANGE_CHANGE_KEYWORDS
    assert I._TIMERANGE_CHANGE_KEYWORDS - own <= set(inspect.signature(S.sample_model).parameters)
    # what timerange_change passes to sample_model itself would collide there: not accepted
    assert not I._TIMERANGE_CHANGE_KEYWORDS & {"mask", "model", "device", "temperature", "condition", "initial_code",
                                               "batch_size", "return_log_probs", "class_conditioning", "codemap_size"}
