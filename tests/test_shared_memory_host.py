"""Host side of variations mode (N rows over one shared encoder memory): the C ABI carries `memory_shared` and the shared
cached-attention entry, and every refusal comes before any GPU call (the models below live on the CPU)."""
import ctypes

import pytest
import torch

from test_batched_inpainting_refusals import ISI_E_INVALID, ISI_E_UNSUPPORTED, _rows, _run, _state
from test_kv16_host import _top


def test_shared_entries_are_exported_and_bound():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    for name in ("isi_rel_attention_decode_shared_f32", "isi_rel_attention_decode_shared_workspace_floats"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    fn = lib.isi_rel_attention_decode_shared_f32
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 5
    assert fn(None, 0, None, 0, None) == ISI_E_INVALID and b"null" in lib.isi_last_error()
    assert lib.isi_rel_attention_decode_shared_workspace_floats(32, 8, 64) >= 32 * 8 * 8 * (64 + 2)


def test_prior_state_carries_memory_shared():
    """The field sits in the four bytes that padded `start_len`: the struct keeps its size and every other offset."""
    from interactive_spectrogram_inpainting import _hip
    st = _hip.isi_prior_state
    assert ctypes.sizeof(st) == _hip.lib().isi_abi_struct_bytes(10)
    assert ("memory_shared", ctypes.c_int) in st._fields_
    assert st.memory_shared.offset == st.start_len.offset + 4
    assert st.cross_out.offset == st.memory_shared.offset + 4 and st.cross_out.offset % 8 == 0
    assert st().memory_shared == 0                                                # the default: a batch dimension


def _attn_args(k_sb):
    from interactive_spectrogram_inpainting import _hip
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    a = _hip.isi_attn_args()
    a.q = a.k = a.v = a.out = p
    a.Sq, a.Sk, a.B, a.H, a.head_dim = 1, 4, 2, 1, 16
    a.q_sb, a.q_sh, a.k_ss, a.k_sb, a.k_sh = 16, 16, 16, k_sb, 16
    a.v_ss, a.v_sb, a.v_sh, a.o_sb, a.o_sh = 16, k_sb, 16, 16, 16
    a.Cq, a.Ck, a.Ek, a.scale = 1, 1, 4, 0.25
    return a, buf


def test_shared_entry_refuses_a_batch_stride_and_bad_formats_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    a, _buf = _attn_args(k_sb=16)
    assert lib.isi_rel_attention_decode_shared_f32(ctypes.byref(a), 3, None, 0, None) == ISI_E_INVALID
    assert b"k_sb" in lib.isi_last_error()
    a, _buf = _attn_args(k_sb=0)
    assert lib.isi_rel_attention_decode_shared_f32(ctypes.byref(a), 3, None, 2, None) == ISI_E_INVALID
    assert b"kv_format" in lib.isi_last_error()
    a.head_dim = 24
    assert lib.isi_rel_attention_decode_shared_f32(ctypes.byref(a), 3, None, 0, None) == ISI_E_UNSUPPORTED
    a.head_dim, a.B = 16, 257
    assert lib.isi_rel_attention_decode_shared_f32(ctypes.byref(a), 3, None, 0, None) == ISI_E_UNSUPPORTED


def test_ragged_plan_refuses_memory_shared_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    w, st, _buf = _state()
    r, _keep = _rows([[3, 5], [4, 6], [4, 7]], [[1, 1], [1, 0], [0, 1]])
    st.memory_shared = 1
    assert _run(w, st, r) == ISI_E_UNSUPPORTED and b"memory_shared" in lib.isi_last_error()
    st.memory_shared = 2
    st.mask = ctypes.addressof(_buf)
    assert lib.isi_prior_sample_run(ctypes.byref(w), ctypes.byref(st), 0, 36, 1.0, 0, 0.0, None) == ISI_E_INVALID
    assert b"memory_shared" in lib.isi_last_error()


def test_sample_model_variations_refusals_before_any_gpu_call(monkeypatch):
    import sample as S
    m = _top()
    monkeypatch.delenv("ISI_DECODE_KV", raising=False)
    F, T = 8, 4
    init = torch.zeros(1, F, T, dtype=torch.int64)
    mask = torch.zeros(3, F, T, dtype=torch.bool)
    mask[:, :, 1:3] = True
    differing = mask.clone()
    differing[1, :, 3] = True
    kw = dict(initial_code=init, num_variations=3)
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 1, [F, T], 1.0, mask=differing, **kw)
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 1, [F, T], [0.9, 1.0, 1.1], mask=mask, **kw)
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 1, [F, T], 1.0, mask=mask, top_k_sampling_k=torch.tensor([0, 5, 0]), **kw)
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 1, [F, T], 1.0, mask=mask, top_p_sampling_p=[0.8, 0.9, 0.8], **kw)
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 1, [F, T], 1.0, mask=mask, use_predictive_sampling=True, **kw)
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 3, [F, T], 1.0, mask=mask, **kw)                 # batch_size is the request's: 1
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 1, [F, T], 1.0, mask=mask, initial_code=init.repeat(3, 1, 1), num_variations=3)
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 1, [F, T], 1.0, mask=mask, uniforms=torch.zeros(32, 2), **kw)
    with pytest.raises(ValueError, match="num_variations"):
        S.sample_model(m, "cpu", 1, [F, T], 1.0, mask=mask, initial_code=init, num_variations=0)
    with pytest.raises(ValueError, match="kv_cache_dtype"):                       # the cache format applies as usual
        S.sample_model(m, "cpu", 1, [F, T], 1.0, mask=mask, kv_cache_dtype=torch.float16, **kw)


def test_native_sampler_refuses_a_batched_memory_as_shared():
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    m = _top()
    S_t, d = m.target_transformer_sequence_length_with_start_symbol, m.d_model
    with pytest.raises(ValueError, match="shared_memory"):
        NativeSampler(m, torch.zeros(S_t, 2, d), torch.zeros(S_t, 2, d), torch.zeros(2, 32, dtype=torch.int64), [True] * 32,
                      torch.zeros(32, 2), shared_memory=True)
