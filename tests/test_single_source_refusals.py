"""CPU-side refusals of single-source cross-attention sampling (aligned decoder / identity memory mask): the checks run on
the host before anything is launched or allocated on a device."""
import ctypes

import pytest
import torch

SMALL = dict(n_class=32, channel=8, kernel_size=5, n_block=1, n_res_block=1, res_channel=8,
             d_model=64, embeddings_dim=8, positional_embeddings_dim=8,
             use_relative_transformer=True, predict_frequencies_first=True,
             conditional_model=True, class_conditioning_prepend_to_dummy_input=True,
             class_conditioning_num_classes_per_modality={"instrument_family_str": 11, "pitch": 61},
             class_conditioning_embedding_dim_per_modality={"instrument_family_str": 16, "pitch": 16},
             conditional_model_nhead=4, conditional_model_num_encoder_layers=1,
             conditional_model_num_decoder_layers=2)


def _state(S_t, S_src, B=2, d=64):
    """An isi_prior_w / isi_prior_state pair with host placeholders behind every pointer (never dereferenced: the calls
    below must return before any launch)."""
    from interactive_spectrogram_inpainting import _hip
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    w = _hip.isi_prior_w()
    w.d_model, w.nhead, w.dim_feedforward, w.n_layers, w.n_class = d, 4, 128, 1, 32
    w.Cd, w.Ed, w.Ce, w.Ee = 4, S_t // 4, 1, S_src
    st = _hip.isi_prior_state()
    st.x_seq = st.kv_cache = st.codes = st.mask = st.uniforms = st.scratch = st.cross_out = p
    st.memory_kv = None
    st.scratch_floats = 1 << 40
    st.S_t, st.S_src, st.S, st.B, st.start_len = S_t, S_src, S_t - 4, B, 4
    return w, st, buf


def test_sample_run_refuses_too_few_source_rows_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    w, st, _buf = _state(S_t=36, S_src=8)            # rows 32 .. 35 would read source row 8
    assert lib.isi_prior_sample_run(ctypes.byref(w), ctypes.byref(st), 0, 36, 1.0, 0, 0.0, None) == -1
    assert b"source row" in lib.isi_last_error()
    w.Ce = 2                                           # source events of two tokens: not built
    st.S_src = 9
    assert lib.isi_prior_sample_run(ctypes.byref(w), ctypes.byref(st), 0, 36, 1.0, 0, 0.0, None) == -4
    w.Ce = 1
    st.cross_out = None                                # the all-rows form needs memory_kv
    assert lib.isi_prior_sample_run(ctypes.byref(w), ctypes.byref(st), 0, 36, 1.0, 0, 0.0, None) == -1
    assert b"null" in lib.isi_last_error()


def test_native_sampler_refuses_misaligned_geometry():
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    from interactive_spectrogram_inpainting.priors.transformer import UpsamplingVQTransformer
    torch.manual_seed(0)
    m = UpsamplingVQTransformer(shape=[16, 8], condition_shape=[8, 4], use_aligned_decoder=True, **SMALL).eval()
    S_t, B, d = m.target_transformer_sequence_length_with_start_symbol, 1, m.d_model
    assert S_t == 132 and m.target_num_channels == 4
    x = torch.zeros(S_t, B, d)
    short = torch.zeros(20, B, d)                      # 33 target events against 20 source rows
    with pytest.raises(ValueError):
        NativeSampler(m, short, x, torch.zeros(B, 128, dtype=torch.int64), [True] * 128, torch.zeros(128, B))


def test_identity_mask_refusals():
    from interactive_spectrogram_inpainting.priors._decode import IncrementalDecoder, NativeSampler
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer
    torch.manual_seed(0)
    m = SelfAttentiveVQTransformer(shape=[8, 4], condition_shape=[8, 4], self_conditional_model=True,
                                   add_mask_token_to_symbols=True, use_identity_memory_mask=True, **SMALL).eval()
    S_t, B, d = m.target_transformer_sequence_length_with_start_symbol, 1, m.d_model
    memory = torch.zeros(S_t, B, d)
    with pytest.raises(NotImplementedError):           # its cached cross-attention reads every memory row
        IncrementalDecoder(m, memory, B)
    with pytest.raises(ValueError):                    # the full forward fails for these shapes too
        NativeSampler(m, torch.zeros(S_t - 1, B, d), torch.zeros(S_t, B, d), torch.zeros(B, 32, dtype=torch.int64),
                      [True] * 32, torch.zeros(32, B))
