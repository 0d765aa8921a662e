"""Host side of the bf16 key/value cache switch: the C ABI carries it, and every refusal comes before any GPU call (the
models below live on the CPU; a launch would fail differently)."""
import ctypes

import pytest
import torch

from test_single_source_refusals import SMALL, _state


def _top():
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer
    torch.manual_seed(0)
    return SelfAttentiveVQTransformer(shape=[8, 4], condition_shape=[8, 4], self_conditional_model=True,
                                      add_mask_token_to_symbols=True, **SMALL).eval()


def test_kv16_entry_is_exported_and_bound():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    assert "isi_rel_attention_decode_kv16_f32" in _hip.SIGNATURES
    fn = lib.isi_rel_attention_decode_kv16_f32
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 4
    assert fn(None, 0, None, None) == -1 and b"null" in lib.isi_last_error()      # ISI_E_INVALID before any launch
    assert (_hip.ISI_KV_F32, _hip.ISI_KV_BF16) == (0, 1)


def test_prior_state_binding_matches_the_library():
    from interactive_spectrogram_inpainting import _hip
    assert ctypes.sizeof(_hip.isi_prior_state) == _hip.lib().isi_abi_struct_bytes(10)
    assert _hip.isi_prior_state._fields_[-1] == ("kv_format", ctypes.c_int)
    assert _hip.isi_prior_state().kv_format == _hip.ISI_KV_F32                     # the default is fp32


def test_sample_run_refuses_unknown_kv_format_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    w, st, _buf = _state(S_t=36, S_src=9)
    for bad in (2, -1, 16):
        st.kv_format = bad
        assert lib.isi_prior_sample_run(ctypes.byref(w), ctypes.byref(st), 0, 36, 1.0, 0, 0.0, None) == -1
        assert b"kv_format" in lib.isi_last_error()


def test_sample_model_refuses_other_formats_before_any_gpu_call(monkeypatch):
    import sample as S
    m = _top()
    monkeypatch.delenv("ISI_DECODE_KV", raising=False)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        S.sample_model(m, "cpu", 1, [8, 4], 1.0, kv_cache_dtype=torch.float16)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        S.sample_model(m, "cpu", 1, [8, 4], 1.0, kv_cache_dtype=torch.int8)
    monkeypatch.setenv("ISI_DECODE_KV", "int8")
    with pytest.raises(ValueError, match="ISI_DECODE_KV"):
        S.sample_model(m, "cpu", 1, [8, 4], 1.0)
    with pytest.raises(ValueError, match="kv_cache_dtype"):                      # an explicit keyword does not read the switch
        S.sample_model(m, "cpu", 1, [8, 4], 1.0, kv_cache_dtype=torch.float16)


def test_predictive_sampling_refuses_a_cache_format(monkeypatch):
    import sample as S
    m = _top()
    monkeypatch.delenv("ISI_DECODE_KV", raising=False)
    with pytest.raises(ValueError, match="predictive"):
        S.sample_model(m, "cpu", 1, [8, 4], 1.0, use_predictive_sampling=True, kv_cache_dtype=torch.bfloat16)
    monkeypatch.setenv("ISI_DECODE_KV", "bf16")
    with pytest.raises(ValueError, match="predictive"):
        S.sample_model(m, "cpu", 1, [8, 4], 1.0, use_predictive_sampling=True)


def test_samplers_refuse_other_dtypes_before_allocating():
    from interactive_spectrogram_inpainting.priors._decode import IncrementalDecoder, NativeSampler, kv_cache_format
    assert kv_cache_format(torch.float32) == 0 and kv_cache_format(torch.bfloat16) == 1
    m = _top()
    S_t, d = m.target_transformer_sequence_length_with_start_symbol, m.d_model
    memory = torch.zeros(S_t, 1, d)
    for bad in (torch.float16, torch.float64, None):
        with pytest.raises(ValueError):
            NativeSampler(m, memory, torch.zeros(S_t, 1, d), torch.zeros(1, 32, dtype=torch.int64), [True] * 32,
                          torch.zeros(32, 1), kv_cache_dtype=bad)
        with pytest.raises(ValueError):
            IncrementalDecoder(m, memory, 1, kv_cache_dtype=bad)
