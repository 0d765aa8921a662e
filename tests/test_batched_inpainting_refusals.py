"""CPU-side refusals of ragged-batch sampling (`isi_prior_sample_run_rows`, `sample_model` with per-row masks and
parameters): the checks run on the host before anything is launched or allocated on a device."""
import ctypes

import numpy as np
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

ISI_E_INVALID, ISI_E_UNSUPPORTED = -1, -4


def _state(S_t=36, B=2, d=64):
    """isi_prior_w / isi_prior_state with host placeholders behind every pointer (never dereferenced: every call below
    must return before any launch)."""
    from interactive_spectrogram_inpainting import _hip
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    w = _hip.isi_prior_w()
    w.d_model, w.nhead, w.dim_feedforward, w.n_layers, w.n_class = d, 4, 128, 1, 32
    w.Cd, w.Ed, w.Ce, w.Ee = 1, S_t, 1, S_t
    st = _hip.isi_prior_state()
    st.x_seq = st.kv_cache = st.memory_kv = st.codes = st.uniforms = st.scratch = p
    st.mask = None                                     # not read by the ragged entry
    st.scratch_floats = 1 << 40
    st.S_t, st.S_src, st.S, st.B, st.start_len = S_t, S_t, S_t - 1, B, 1
    return w, st, buf


def _rows(pos, commit):
    from interactive_spectrogram_inpainting import _hip
    pos = np.ascontiguousarray(np.asarray(pos, dtype=np.int32))
    commit = np.ascontiguousarray(np.asarray(commit, dtype=np.uint8))
    r = _hip.isi_prior_rows()
    r.pos = r.commit = 16                              # device arrays: never read on the host
    r.pos_host, r.commit_host = pos.ctypes.data, commit.ctypes.data
    r.n_steps = pos.shape[0]
    return r, (pos, commit)


def _run(w, st, r, t_end=None):
    from interactive_spectrogram_inpainting import _hip
    return _hip.lib().isi_prior_sample_run_rows(ctypes.byref(w), ctypes.byref(st), ctypes.byref(r) if r is not None else None,
                                                0, t_end if t_end is not None else (r.n_steps if r is not None else 1), 1.0, 0, 0.0, None)


def test_rows_struct_abi():
    from interactive_spectrogram_inpainting import _hip
    assert _hip.lib().isi_abi_struct_bytes(13) == ctypes.sizeof(_hip.isi_prior_rows)


def test_sample_run_rows_refuses_bad_plans_before_any_launch():
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    w, st, _buf = _state()
    good_pos, good_commit = [[3, 5], [4, 6], [4, 7]], [[1, 1], [1, 0], [0, 1]]
    r, keep = _rows([[3, 36], [4, 36]], [[0, 0], [0, 0]])               # position S_t: out of range
    assert _run(w, st, r) == ISI_E_INVALID and b"position" in lib.isi_last_error()
    r, keep = _rows([[3, -1], [4, 0]], [[0, 0], [0, 0]])                # negative position
    assert _run(w, st, r) == ISI_E_INVALID
    r, keep = _rows([[3, 5], [2, 6]], [[0, 0], [0, 0]])                 # a row moves back
    assert _run(w, st, r) == ISI_E_INVALID and b"0 or 1" in lib.isi_last_error()
    r, keep = _rows([[3, 5], [5, 6]], [[0, 0], [0, 0]])                 # a row skips a position
    assert _run(w, st, r) == ISI_E_INVALID
    st.start_len = 4                                                     # token index = position - 3
    r, keep = _rows([[2, 5], [3, 6]], [[1, 0], [0, 0]])                 # commit at token -1
    assert _run(w, st, r) == ISI_E_INVALID and b"commit" in lib.isi_last_error()
    st.S = 3
    r, keep = _rows([[2, 5], [3, 6]], [[0, 0], [0, 1]])                 # commit at token 3 = S
    assert _run(w, st, r) == ISI_E_INVALID
    st.start_len, st.S = 1, 35
    r, keep = _rows(good_pos, good_commit)
    assert _run(w, st, r, t_end=4) == ISI_E_INVALID                      # steps beyond the plan
    assert _run(w, st, None) == ISI_E_INVALID                            # NULL pointers
    r.pos_host = None
    assert _run(w, st, r) == ISI_E_INVALID
    r, keep = _rows(good_pos, good_commit)
    r.commit = None
    assert _run(w, st, r) == ISI_E_INVALID
    r, keep = _rows(good_pos, good_commit)
    st.codes = None
    assert _run(w, st, r) == ISI_E_INVALID
    st.codes = st.x_seq
    for B in (0, 257):                                                   # batch sizes: as isi_prior_sample_run
        st.B = B
        r, keep = _rows(np.zeros((2, max(B, 1))), np.zeros((2, max(B, 1))))
        assert _run(w, st, r) == ISI_E_UNSUPPORTED


def _top():
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer
    torch.manual_seed(0)
    return SelfAttentiveVQTransformer(shape=[8, 4], condition_shape=[8, 4], self_conditional_model=True,
                                      add_mask_token_to_symbols=True, **SMALL).eval()


def test_sample_model_refusals():
    import sample as S
    m = _top()
    B = 3
    init = torch.zeros(B, 8, 4, dtype=torch.int64)
    masks = torch.zeros(B, 8, 4, dtype=torch.bool)
    masks[0, :, 1] = True
    masks[1, 2:5, 3] = True
    with pytest.raises(ValueError):              # a mask for 2 rows, a batch of 3
        S.sample_model(m, "cpu", B, [8, 4], 1.0, initial_code=init, mask=masks[:2])
    with pytest.raises(ValueError):              # per-row parameters of the wrong length
        S.sample_model(m, "cpu", B, [8, 4], [1.0, 0.9], initial_code=init, mask=masks)
    with pytest.raises(ValueError):
        S.sample_model(m, "cpu", B, [8, 4], 1.0, initial_code=init, mask=masks, top_k_sampling_k=torch.tensor([1, 2]))
    with pytest.raises(ValueError):
        S.sample_model(m, "cpu", B, [8, 4], 1.0, initial_code=init, mask=masks, top_p_sampling_p=[0.5, 0.6, 0.7, 0.8])
    with pytest.raises(ValueError):              # predictive sampling walks every row at the same positions
        S.sample_model(m, "cpu", B, [8, 4], 1.0, initial_code=init, mask=masks, use_predictive_sampling=True)


def test_ragged_plan_walks_each_rows_own_span():
    import sample as S
    S_len, i_off = 10, 2
    mask = np.zeros((3, S_len), dtype=bool)
    mask[0, 2:5] = True                 # positions 4 .. 6
    mask[1, [6, 9]] = True              # positions 8 .. 11, commits at 8 and 11
    pos, commit, prefill = S._ragged_plan(mask, i_off)
    assert prefill == 8 and pos.shape == (4, 3)
    assert pos[:, 0].tolist() == [4, 5, 6, 6] and commit[:, 0].tolist() == [1, 1, 1, 0]
    assert pos[:, 1].tolist() == [8, 9, 10, 11] and commit[:, 1].tolist() == [1, 0, 0, 1]
    assert pos[:, 2].tolist() == [0, 0, 0, 0] and not commit[:, 2].any()      # nothing masked: idles, never commits
