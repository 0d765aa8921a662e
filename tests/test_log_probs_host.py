"""Host side of per-token log-probabilities: the C ABI carries `isi_prior_state.token_log_probs` and the two new entries, and
every refusal comes before any GPU call (the models below live on the CPU; a launch would fail differently)."""
import ctypes

import pytest
import torch

from test_single_source_refusals import SMALL

ISI_E_INVALID = -1


def _top():
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer
    torch.manual_seed(0)
    return SelfAttentiveVQTransformer(shape=[8, 4], condition_shape=[8, 4], self_conditional_model=True,
                                      add_mask_token_to_symbols=True, **SMALL).eval()


def _bottom():
    from interactive_spectrogram_inpainting.priors.transformer import UpsamplingVQTransformer
    torch.manual_seed(0)
    return UpsamplingVQTransformer(shape=[16, 8], condition_shape=[8, 4], **SMALL).eval()


def test_token_log_prob_entry_is_exported_bound_and_checks_its_arguments():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    assert "isi_token_log_prob_f32" in _hip.SIGNATURES
    fn = lib.isi_token_log_prob_f32
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7
    buf = (ctypes.c_float * 64)()
    codes = (ctypes.c_int64 * 4)()
    p, c = ctypes.addressof(buf), ctypes.addressof(codes)
    # (host placeholders behind the pointers: every call below must return before any launch)
    bad = [(None, 8, 2, 8, c, p), (p, 8, 2, 8, None, p), (p, 8, 2, 8, c, None),      # null pointers
           (p, 8, 0, 8, c, p), (p, 8, -1, 8, c, p),                                  # rows <= 0
           (p, 8, 2, 0, c, p), (p, 8, 2, -3, c, p),                                  # n <= 0
           (p, 7, 2, 8, c, p), (p, 0, 2, 8, c, p)]                                   # stride < n
    for args in bad:
        assert fn(*args, None) == ISI_E_INVALID, args
        assert b"token_log_prob" in lib.isi_last_error(), args


def test_sample_row_log_prob_entry_is_exported_bound_and_checks_its_arguments():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    assert "isi_sample_row_log_prob_f32" in _hip.SIGNATURES
    fn = lib.isi_sample_row_log_prob_f32
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 11
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert fn(p, 8, 2, 8, 1.0, 0, 0.0, p, p, None, None) == ISI_E_INVALID           # no destination for the log-probability
    assert b"sample_row_log_prob" in lib.isi_last_error()
    assert fn(p, 7, 2, 8, 1.0, 0, 0.0, p, p, p, None) == ISI_E_INVALID              # stride < n
    assert fn(p, 8, 2, 8, 0.0, 0, 0.0, p, p, p, None) == ISI_E_INVALID              # temperature <= 0


def test_prior_state_appends_token_log_probs():
    """The field is the last one, behind kv_format; every other offset is the parent layout's (7 pointers, a size_t, 6 ints,
    a pointer, an int: memory_shared at 84, cross_out at 88, kv_format at 96, 104 bytes), and the library agrees on the size."""
    from interactive_spectrogram_inpainting import _hip
    st = _hip.isi_prior_state
    assert _hip._PRIOR_STATE_APPENDED[-1] == ("token_log_probs", ctypes.c_void_p)
    assert ctypes.sizeof(st) == _hip.lib().isi_abi_struct_bytes(10)
    # the last field of the layout: it ends where the struct ends and lies behind every other field
    assert st.token_log_probs.offset + st.token_log_probs.size == ctypes.sizeof(st)
    assert all(getattr(st, name).offset < st.token_log_probs.offset for name, _ in st._fields_)
    assert (st.memory_shared.offset, st.cross_out.offset, st.kv_format.offset) == (84, 88, 96)
    assert st.token_log_probs.offset % 8 == 0 and st.token_log_probs.offset > st.kv_format.offset
    assert st.token_log_probs.offset == 104 and ctypes.sizeof(st) == 112
    assert st().token_log_probs is None                                              # a zeroed struct: off


def test_predictive_sampling_refuses_log_probs():
    import sample as S
    m = _top()
    with pytest.raises(ValueError, match="return_log_probs"):
        S.sample_model(m, "cpu", 1, [8, 4], 1.0, use_predictive_sampling=True, return_log_probs=True)
    with pytest.raises(ValueError, match="return_log_probs"):                        # ... before num_variations is looked at
        S.sample_model(m, "cpu", 1, [8, 4], 1.0, use_predictive_sampling=True, return_log_probs=True, num_variations=4)


def test_timerange_change_refuses_scores_it_cannot_give():
    import inpainting as I
    top, bottom = _top(), _bottom()
    top_code = torch.zeros(1, 8, 4, dtype=torch.int64)
    bottom_code = torch.zeros(1, 16, 8, dtype=torch.int64)
    mask = torch.zeros(1, 8, 4, dtype=torch.bool)
    mask[0, 2:4, 1:3] = True
    cls = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}
    args = (top, bottom, top_code, bottom_code, mask, "top", 0, 1.0, cls, cls, "cpu")
    for extra in ({}, {"num_variations": 3}):
        with pytest.raises(ValueError, match="uniform_sampling"):
            I.timerange_change(*args, uniform_sampling=True, return_scores=True, **extra)
        with pytest.raises(ValueError, match="return_scores"):
            I.timerange_change(*args, sort_by_likelihood=True, **extra)
    req = dict(top_code=top_code, bottom_code=bottom_code, mask=mask, layer="top", start_index_top=0, temperature=1.0,
               class_conditioning_top=cls, class_conditioning_bottom=cls, uniform_sampling=True)
    with pytest.raises(ValueError, match="uniform_sampling"):
        I.timerange_change_batch(top, bottom, [req], "cpu", return_scores=True)


def test_native_sampler_takes_the_option():
    """`log_probs` is a keyword of NativeSampler; a refusal that comes before any allocation still comes first."""
    import inspect
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    assert inspect.signature(NativeSampler.__init__).parameters["log_probs"].default is False
    m = _top()
    S_t, d = m.target_transformer_sequence_length_with_start_symbol, m.d_model
    with pytest.raises(ValueError):
        NativeSampler(m, torch.zeros(S_t, 1, d), torch.zeros(S_t, 1, d), torch.zeros(1, 32, dtype=torch.int64), [True] * 32,
                      torch.zeros(32, 1), kv_cache_dtype=torch.float16, log_probs=True)
