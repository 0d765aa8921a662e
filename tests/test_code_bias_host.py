"""Host side of code palettes and logit bias in prior sampling: the float64 specification of the biased draw (the
specification of tests/tests_support.py on float32(logits + bias)), the layout of `isi_prior_code_bias` beside an unchanged
`isi_prior_state`, the new C entries and every refusal -- of the library with ISI_E_INVALID before any launch, of Python with a
ValueError before any GPU work (the models below live on the CPU; a launch would fail differently).  The bias rows of
tests/test_code_bias_gpu.py are generated here, and shown here to leave at least 90 % of the cases resolvable."""
import ctypes

import numpy as np
import pytest
import torch

import tests_support as TS
from test_single_source_refusals import SMALL

ISI_E_INVALID = -1
BIAS_KINDS = ("zeros", "half_banned", "one_class", "dense3", "lowest+20", "argmax_banned")
NEG = np.float32(-np.inf)
TOP_U = np.nextafter(np.float32(1.0), np.float32(0.0))        # the largest float32 below 1


def bias_rows(logits, seed):
    """The six bias rows a logit row is crossed with: {kind: float32 [n]}, seeded by `seed` alone.  The half-banned palette
    always keeps the row's argmax (a finite class stays); the one-class palette is a class with a finite logit."""
    n = logits.shape[0]
    g = np.random.default_rng(seed)
    finite = np.flatnonzero(np.isfinite(logits))
    top = int(np.argmax(logits))
    low = int(finite[np.argmin(logits[finite])])
    half = np.zeros(n, dtype=np.float32)
    half[g.permutation(n)[:n // 2]] = NEG
    half[top] = 0.0
    one = np.full(n, NEG, dtype=np.float32)
    one[int(finite[g.integers(finite.shape[0])])] = 0.0
    dense = np.asarray(3.0 * g.standard_normal(n), dtype=np.float32)
    plus = np.zeros(n, dtype=np.float32)
    plus[low] = 20.0
    ban = np.zeros(n, dtype=np.float32)
    ban[top] = NEG
    return dict(zip(BIAS_KINDS, (np.zeros(n, dtype=np.float32), half, one, dense, plus, ban)))


def biased_cases(n):
    """(cases, generated): every case of TS.sampling_cases(n) crossed with the six bias rows, as (case with the top_p picked
    again for the BIASED row, kind, bias, biased float32 logits).  A case whose biased row has no finite logit (outside the
    contract) or makes TS.sampling_pick_top_p return None is left out; `generated` counts all of them."""
    cases, generated = [], 0
    for ci, c in enumerate(TS.sampling_cases(n)):
        what = c.name.rsplit("/p", 1)[1]
        what = float(what) if what[0].isdigit() else what
        for kind, bias in bias_rows(c.logits, 1000 * n + ci).items():
            generated += 1
            biased = (c.logits + bias).astype(np.float32)
            if not np.isfinite(biased).any():
                continue
            top_p = TS.sampling_pick_top_p(biased, c.temperature, c.top_k, what)
            if top_p is None:
                continue
            cases.append((c._replace(top_p=top_p), kind, bias, biased))
    return cases, generated


@pytest.mark.parametrize("n", [2, 64, 65, 513, 1024])
def test_bias_rows_leave_nine_cases_in_ten(n):
    """The specification alone, for the seeds of the GPU test: at least 90 % of the generated (case, bias) pairs stay."""
    cases, generated = biased_cases(n)
    kinds = {k: sum(1 for _, kind, _, _ in cases if kind == k) for k in BIAS_KINDS}
    print(f"n={n}: {len(cases)} of {generated} biased cases kept; per kind {kinds}")
    assert len(cases) >= 0.9 * generated, (n, len(cases), generated)
    assert all(kinds.values())


@pytest.mark.parametrize("n", [2, 65, 513, 1024])
def test_biased_specification(n):
    """TS.sampling_spec(float32(logits + bias)): a class with bias -inf is never kept, a zero bias gives the unbiased
    specification, and the float64 draw returns no banned class at u = 0 and at the largest float32 below 1."""
    u = np.array([0.0, TOP_U], dtype=np.float32)
    for ri, (name, logits, t) in enumerate(TS.sampling_rows(n)):
        for kind, bias in bias_rows(logits, 77 * n + ri).items():
            biased = (logits + bias).astype(np.float32)
            if not np.isfinite(biased).any():
                continue
            for k, p in ((0, 0.0), (5, 0.0), (0, 0.8), (40, 0.9)):
                spec = TS.sampling_spec(biased, t, k, p)
                banned = bias == NEG
                assert not spec.kept[banned].any(), (name, kind, k, p)
                assert not spec.prob[banned].any()
                drawn = TS.sampling_float64_draw(spec, u)
                assert not banned[drawn].any(), (name, kind, k, p, drawn)
                if kind == "zeros":
                    plain = TS.sampling_spec(logits, t, k, p)
                    assert np.array_equal(spec.kept, plain.kept) and np.array_equal(spec.cdf, plain.cdf)
                    assert np.array_equal(spec.lg.view(np.int32), plain.lg.view(np.int32))
                if kind == "one_class":
                    assert int(spec.kept.sum()) == 1 and drawn[0] == drawn[1] == int(np.flatnonzero(bias == 0.0)[0])


# ---------------------------------------------------------------- the C ABI

class _ParentState(ctypes.Structure):
    """`isi_prior_state` as it was before the code-bias fields, written out."""
    _fields_ = [("x_seq", ctypes.c_void_p), ("kv_cache", ctypes.c_void_p), ("memory_kv", ctypes.c_void_p),
                ("codes", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("uniforms", ctypes.c_void_p),
                ("scratch", ctypes.c_void_p), ("scratch_floats", ctypes.c_size_t), ("S_t", ctypes.c_int),
                ("S_src", ctypes.c_int), ("S", ctypes.c_int), ("B", ctypes.c_int), ("start_len", ctypes.c_int),
                ("memory_shared", ctypes.c_int), ("cross_out", ctypes.c_void_p), ("kv_format", ctypes.c_int),
                ("token_log_probs", ctypes.c_void_p)]


NEW_FIELDS = ("code_bias", "code_bias_index", "code_bias_count", "code_bias_batch")


def test_code_bias_struct_beside_an_unchanged_prior_state():
    """tests/test_log_probs_host.py pins `isi_prior_state` at 112 bytes with `token_log_probs` as its last field, so the
    four fields cannot be appended to it: they form `isi_prior_code_bias`, passed beside the state.  `isi_prior_state` is
    byte for byte the parent's (size, and the offset and size of every field, against the replica above), the new struct
    holds the four fields in the header's order, the library agrees on both sizes, and a zeroed struct has the option off."""
    from interactive_spectrogram_inpainting import _hip
    st, cb = _hip.isi_prior_state, _hip.isi_prior_code_bias
    assert ctypes.sizeof(st) == _hip.lib().isi_abi_struct_bytes(10) == ctypes.sizeof(_ParentState)
    for name, _ in _ParentState._fields_:                                  # every earlier field where it was
        assert getattr(st, name).offset == getattr(_ParentState, name).offset, name
        assert getattr(st, name).size == getattr(_ParentState, name).size, name
    assert not any(hasattr(st, name) for name in NEW_FIELDS)
    assert ctypes.sizeof(cb) == _hip.lib().isi_abi_struct_bytes(14) == 24
    assert [name for name, _ in cb._fields_] == list(NEW_FIELDS)
    assert [getattr(cb, name).offset for name in NEW_FIELDS] == [0, 8, 16, 20]
    z = cb()                                                               # a zeroed struct: off
    assert z.code_bias is None and z.code_bias_index is None and z.code_bias_count == 0 and z.code_bias_batch == 0


def test_sample_row_bias_entry_is_exported_bound_and_checks_its_arguments():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    assert "isi_sample_row_bias_f32" in _hip.SIGNATURES
    fn = lib.isi_sample_row_bias_f32
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    # (host placeholders behind the pointers: every call below must return before any launch)
    #        logits stride rows n  T    k  p    u  out filtered bias stride count rows
    bad = [(p, 8, 2, 8, 1.0, 0, 0.0, p, p, None, None, 8, 1, None),       # no table
           (p, 8, 2, 8, 1.0, 0, 0.0, p, p, None, p, 8, 0, None),          # bias_count <= 0
           (p, 8, 2, 8, 1.0, 0, 0.0, p, p, None, p, 8, -2, p),
           (p, 8, 2, 8, 1.0, 0, 0.0, p, p, None, p, 7, 1, None),          # bias_stride < n
           (p, 7, 2, 8, 1.0, 0, 0.0, p, p, None, p, 8, 1, None),          # the existing ones: stride < n,
           (None, 8, 2, 8, 1.0, 0, 0.0, p, p, None, p, 8, 1, None),       # null pointers,
           (p, 8, 2, 8, 1.0, 0, 0.0, None, p, None, p, 8, 1, None),
           (p, 8, 2, 8, 1.0, 0, 0.0, p, None, None, p, 8, 1, None),
           (p, 8, 0, 8, 1.0, 0, 0.0, p, p, None, p, 8, 1, None),          # rows <= 0, n <= 0, temperature <= 0
           (p, 8, 2, 0, 1.0, 0, 0.0, p, p, None, p, 8, 1, None),
           (p, 8, 2, 8, 0.0, 0, 0.0, p, p, None, p, 8, 1, None)]
    for args in bad:
        assert fn(*args, None) == ISI_E_INVALID, args
        assert b"sample_row" in lib.isi_last_error(), args


def test_loop_entries_refuse_inconsistent_code_bias_fields():
    """Exactly one of the two pointers, a count <= 0, a batch that is neither 1 nor B: ISI_E_INVALID from both loop entries,
    before anything else of the state is looked at (the state below holds nothing else).  NULL and a zeroed struct are
    the option off: the call goes on to the checks of the entry without the argument."""
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    for name in ("isi_prior_sample_run_bias", "isi_prior_sample_run_rows_bias"):
        assert name in _hip.SIGNATURES and getattr(lib, name).restype is ctypes.c_int
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    w = _hip.isi_prior_w()
    w.n_layers, w.d_model, w.nhead, w.n_class = 1, 64, 4, 8
    rows = _hip.isi_prior_rows()
    st = _hip.isi_prior_state()
    st.B, st.S, st.S_t, st.start_len = 3, 4, 5, 2
    for table, index, count, batch in ((p, None, 1, 1), (None, p, 1, 1), (p, p, 0, 1), (p, p, -1, 1), (p, p, 2, 0),
                                       (p, p, 2, 2), (p, p, 2, 4)):
        cb = _hip.isi_prior_code_bias()
        cb.code_bias, cb.code_bias_index, cb.code_bias_count, cb.code_bias_batch = table, index, count, batch
        assert lib.isi_prior_sample_run_bias(ctypes.byref(w), ctypes.byref(st), ctypes.byref(cb), 0, 1, 1.0, 0, 0.0,
                                             None) == ISI_E_INVALID
        assert b"code_bias" in lib.isi_last_error(), (count, batch)
        assert lib.isi_prior_sample_run_rows_bias(ctypes.byref(w), ctypes.byref(st), ctypes.byref(rows), ctypes.byref(cb), 0, 0,
                                                  1.0, 0, 0.0, None) == ISI_E_INVALID
        assert b"code_bias" in lib.isi_last_error(), (count, batch)
    for cb in (None, ctypes.byref(_hip.isi_prior_code_bias())):            # off: the plain entry's own refusal (no state arrays)
        assert lib.isi_prior_sample_run_bias(ctypes.byref(w), ctypes.byref(st), cb, 0, 1, 1.0, 0, 0.0, None) == ISI_E_INVALID
        assert b"code_bias" not in lib.isi_last_error() and b"null state pointer" in lib.isi_last_error()


# ---------------------------------------------------------------- Python

def _top():
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer
    torch.manual_seed(0)
    return SelfAttentiveVQTransformer(shape=[8, 4], condition_shape=[8, 4], self_conditional_model=True,
                                      add_mask_token_to_symbols=True, **SMALL).eval()


def _bottom():
    from interactive_spectrogram_inpainting.priors.transformer import UpsamplingVQTransformer
    torch.manual_seed(0)
    return UpsamplingVQTransformer(shape=[16, 8], condition_shape=[8, 4], **SMALL).eval()


def test_codes_in_use_against_numpy_unique():
    import sample as S
    g = torch.Generator().manual_seed(4)
    a = torch.randint(0, 40, (1, 8, 10), generator=g)
    b = torch.randint(100, 130, (3, 16, 20), generator=g)
    for maps in (a, b, [a, b], (a,)):
        got = S.codes_in_use(maps, 512)
        assert got.dtype == torch.bool and tuple(got.shape) == (512,)
        every = np.concatenate([m.numpy().reshape(-1) for m in ([maps] if torch.is_tensor(maps) else maps)])
        assert np.array_equal(np.flatnonzero(got.numpy()), np.unique(every))
    with_mask_token = torch.tensor([[[3, 32, 5]]])                         # the top prior's mask token is not a class
    assert S.codes_in_use(with_mask_token, 32).nonzero().reshape(-1).tolist() == [3, 5]


def test_sample_model_refuses_bad_code_bias_before_any_gpu_work():
    import sample as S
    m = _top()
    n, (F, T) = m.n_class_target, m.shape
    call = lambda **kw: S.sample_model(m, "cpu", 2, [F, T], 1.0, **kw)
    ok = torch.zeros(n)
    rows = torch.zeros(3, n)
    cells = torch.zeros(F, T, dtype=torch.int64)
    bad = [dict(code_bias=ok, allowed_codes=[1, 2]),                       # both
           dict(code_bias=torch.full((n,), float("nan"))),                 # NaN, +inf
           dict(code_bias=ok.clone().index_fill_(0, torch.tensor([4]), float("inf"))),
           dict(code_bias=torch.full((n,), -float("inf"))),                # a row that bans everything
           dict(code_bias=torch.cat([rows[:2], torch.full((1, n), -float("inf"))]), code_bias_map=cells),
           dict(allowed_codes=torch.zeros(n, dtype=torch.bool)),
           dict(allowed_codes=[]),
           dict(code_bias=rows, code_bias_map=cells + 3),                  # an index >= R
           dict(code_bias=rows),                                           # R rows and no map
           dict(code_bias_map=cells),                                      # a map and no table
           dict(code_bias=torch.zeros(n + 1)),                             # width != n_class_target
           dict(code_bias=torch.zeros(2, 3, n), code_bias_map=cells),      # wrong shapes
           dict(code_bias=rows, code_bias_map=torch.zeros(F, T + 1, dtype=torch.int64)),
           dict(code_bias=rows, code_bias_map=torch.zeros(3, F, T, dtype=torch.int64)),     # rows of another batch
           dict(code_bias=rows, code_bias_map=torch.zeros(F, T)),          # a float map
           dict(code_bias=torch.zeros(n, dtype=torch.int64)),              # an integer table
           dict(allowed_codes=torch.ones(n + 1, dtype=torch.bool)),
           dict(allowed_codes=[0, n]), dict(allowed_codes=[-1])]           # class indices out of range
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
        with pytest.raises(ValueError):                                    # the chunked path checks before it splits
            S.sample_model(m, "cpu", 300, [F, T], 1.0, **{k: v for k, v in kw.items()})
    for kw in (dict(code_bias=ok), dict(allowed_codes=[1, 2]), dict(code_bias=rows, code_bias_map=cells)):
        with pytest.raises(ValueError, match="predictive"):
            call(use_predictive_sampling=True, **kw)
        with pytest.raises(ValueError, match="predictive"):
            S.sample_model(m, "cpu", 1, [F, T], 1.0, use_predictive_sampling=True, num_variations=3, **kw)
    with pytest.raises(ValueError):                                        # one request: one map
        S.sample_model(m, "cpu", 1, [F, T], 1.0, num_variations=3, code_bias=rows,
                       code_bias_map=torch.zeros(3, F, T, dtype=torch.int64))


def test_checked_options_become_a_table_and_a_map():
    """allowed_codes is a one-row table of 0 and -inf; a map goes into sequence order the way the mask does."""
    import sample as S
    m = _bottom()
    n, (F, T) = m.n_class_target, m.shape
    table, cells = S._code_bias_rows(m, 2, None, None, {3, 7})
    assert cells is None and tuple(table.shape) == (1, n)
    assert table[0, [3, 7]].tolist() == [0.0, 0.0] and int(torch.isinf(table).sum()) == n - 2 and bool((table <= 0).all())
    mask = torch.zeros(n, dtype=torch.bool)
    mask[[3, 7]] = True
    assert torch.equal(S._code_bias_rows(m, 2, None, None, mask)[0], table)
    assert torch.equal(S._code_bias_index(m, None), torch.zeros(1, F * T, dtype=torch.int32))
    cells = torch.arange(F * T).reshape(1, F, T) % 5 - 1
    table, checked = S._code_bias_rows(m, 2, torch.zeros(4, n), cells, None)
    index = S._code_bias_index(m, checked)
    assert index.dtype == torch.int32 and tuple(index.shape) == (1, F * T)
    assert torch.equal(index.long(), m.target_codemaps_helper.to_sequence(cells))
    assert not torch.equal(index.long().reshape(-1), cells.reshape(-1))    # (the zig-zag order is not the map's)


def test_native_sampler_takes_the_options():
    import inspect
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    par = inspect.signature(NativeSampler.__init__).parameters
    assert par["code_bias"].default is None and par["code_bias_index"].default is None
    from interactive_spectrogram_inpainting.priors import _ops
    par = inspect.signature(_ops.sample_rows).parameters
    assert par["bias"].default is None and par["bias_rows"].default is None


def test_timerange_change_takes_the_options_per_layer():
    import inpainting as I
    top, bottom = _top(), _bottom()
    top_code = torch.zeros(1, 8, 4, dtype=torch.int64)
    bottom_code = torch.zeros(1, 16, 8, dtype=torch.int64)
    mask = torch.zeros(1, 8, 4, dtype=torch.bool)
    mask[0, 2:4, 1:3] = True
    cls = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}
    args = (top, bottom, top_code, bottom_code, mask, "top", 0, 1.0, cls, cls, "cpu")
    assert I._CODE_BIAS_KEYWORDS == {f"{n}_{l}" for n in ("allowed_codes", "code_bias", "code_bias_map") for l in ("top", "bottom")}
    for extra in ({}, {"num_variations": 3}):
        with pytest.raises(TypeError, match="allowed_codes_top"):          # which layer?
            I.timerange_change(*args, allowed_codes=[1], **extra)
        with pytest.raises(ValueError, match="uniform_sampling"):
            I.timerange_change(*args, uniform_sampling=True, allowed_codes_top=[1], **extra)
        with pytest.raises(ValueError):                                    # checked before any GPU work
            I.timerange_change(*args, allowed_codes_top=[], **extra)
        with pytest.raises(ValueError):
            I.timerange_change(*args, code_bias_top=torch.zeros(5), **extra)
    req = dict(top_code=top_code, bottom_code=bottom_code, mask=mask, layer="top", start_index_top=0, temperature=1.0,
               class_conditioning_top=cls, class_conditioning_bottom=cls)
    with pytest.raises(ValueError):
        I.timerange_change_batch(top, bottom, [req, dict(req, code_bias_bottom=torch.zeros(2, 32))], "cpu")
    with pytest.raises(ValueError, match="uniform_sampling"):
        I.timerange_change_batch(top, bottom, [dict(req, uniform_sampling=True, allowed_codes_bottom=[1])], "cpu")
