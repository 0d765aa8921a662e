"""Variations mode: N rows of one request over ONE shared encoder memory.  The cached cross-attention that fetches a key row
once for a block of rows (isi_rel_attention_decode_shared_f32), isi_prior_state.memory_shared in the native loop, and
sample_model(num_variations=N) / inpainting.timerange_change(num_variations=N) on top of it.  The default path
(num_variations=None, memory_shared = 0) is untouched."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_prior_gpu import TOL, _close, _dev, _models, _window_mask
from test_single_source_sampling_gpu import _aligned_bottom, _identity_top

pytestmark = pytest.mark.gpu

CLS = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}


def _formula(q, k, v, rel, H, nk, q_pos, Cq, Ck, Ek):
    """float64 cached attention of B query rows against shared keys / values k, v [S, 1, d] (fp32, or bf16 rows widened):
    s = scale q.(k_j + e_r), r = clamp(q_pos // Cq - j // Ck + Ek - 1, 0, R - 1); softmax over the nk keys; out = sum p_j v_j."""
    B, d = q.shape
    hd = d // H
    hq = q.view(B, H, hd).cpu().double()
    hk = k[:nk, 0].float().view(nk, H, hd).permute(1, 0, 2).cpu().double()           # [H, nk, hd]
    hv = v[:nk, 0].float().view(nk, H, hd).permute(1, 0, 2).cpu().double()
    if rel is not None:
        idx = (q_pos // Cq - torch.arange(nk) // Ck + Ek - 1).clamp(0, rel.shape[1] - 1)
        hk = hk + rel.cpu().double()[:, idx]
    logit = torch.einsum("bhd,hjd->bhj", hq, hk) / math.sqrt(hd)
    return torch.einsum("bhj,hjd->bhd", torch.softmax(logit, -1), hv).reshape(B, d).float()


@pytest.mark.parametrize("kv", ["f32", "bf16"])
@pytest.mark.parametrize("hd,H", [(16, 4), (32, 8), (64, 8)])
def test_shared_attention_against_formula_and_per_row_kernel(hd, H, kv):
    """Test 1 of the issue.  Key counts of 1 / 2 / many splits (tiles of 64 keys, up to 8 splits), B = 1 .. 130 (nine row
    blocks, the last with two rows), self-like geometry and the bottom prior's cross geometry with and without a table.
    Rows beyond the keys in use hold NaN.  Both comparisons at TOL: (a) the float64 formula on the same (rounded) rows,
    (b) the per-row kernel on the keys expanded to B rows."""
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    S = 1100
    d = H * hd
    g = torch.Generator().manual_seed(100 + hd + (kv == "bf16"))
    dt = torch.bfloat16 if kv == "bf16" else torch.float32
    rel = (torch.randn(H, 2 * S - 1, hd, generator=g) * 0.2).to(dev)
    k0 = torch.randn(S, 1, d, generator=g).to(dt).to(dev)
    v0 = torch.randn(S, 1, d, generator=g).to(dt).to(dev)
    worst = 0.0
    for B in (1, 3, 8, 32, 130):
        for nk in (1, 40, 64, 65, 128, 300, 1025):
            k, v = k0.clone(), v0.clone()
            k[nk:] = float("nan")
            v[nk:] = float("nan")
            kB, vB = k.expand(-1, B, -1).contiguous(), v.expand(-1, B, -1).contiguous()
            cases = [("self-like", rel, nk - 1, 1, 1, S), ("cross", rel, min(4 * nk - 1, 2051), 4, 1, nk),
                     ("cross no table", None, 7, 4, 1, nk)]
            for what, r, q_pos, Cq, Ck, Ek in cases:
                q = torch.randn(B, d, generator=g).to(dev)
                got = _ops.rel_attention_decode(q, k, v, r, H, nk, q_pos, Cq, Ck, Ek, shared=True)
                tag = f"hd={hd} {kv} B={B} nk={nk} {what}"
                assert torch.isfinite(got).all(), tag
                ref = _formula(q, k, v, r, H, nk, q_pos, Cq, Ck, Ek)
                row = _ops.rel_attention_decode(q, kB, vB, r, H, nk, q_pos, Cq, Ck, Ek)
                ea = float((got.cpu() - ref).abs().max() / ref.abs().max())
                eb = float((got - row).abs().max() / row.abs().max())
                worst = max(worst, ea, eb)
                _close(got, ref, TOL, f"{tag}: formula")
                _close(got, row, TOL, f"{tag}: per-row kernel on expanded keys")
                if B > 1:                      # [S, 1, d] keys against several query rows route to the shared entry
                    assert torch.equal(_ops.rel_attention_decode(q, k, v, r, H, nk, q_pos, Cq, Ck, Ek), got), tag
    print(f"shared attention hd={hd} {kv}: worst error / max|ref| = {worst:.3e} (bound {TOL:.0e})")


def test_shared_entry_refuses_a_batch_stride():
    """Test 6b: k_sb != 0 -> invalid argument."""
    from interactive_spectrogram_inpainting import _hip
    dev = _dev()
    q = torch.randn(2, 64, device=dev)
    k = torch.randn(16, 2, 64, device=dev)
    out = torch.empty_like(q)
    a = _hip.isi_attn_args()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), k.data_ptr(), out.data_ptr()
    a.Sq, a.Sk, a.B, a.H, a.head_dim = 1, 16, 2, 4, 16
    a.q_sb, a.q_sh, a.k_ss, a.k_sb, a.k_sh = 64, 16, 128, 64, 16
    a.v_ss, a.v_sb, a.v_sh, a.o_sb, a.o_sh = 128, 64, 16, 64, 16
    a.Cq, a.Ck, a.Ek, a.scale = 1, 1, 16, 0.25
    lib = _hip.lib()
    assert lib.isi_rel_attention_decode_shared_f32(ctypes.byref(a), 15, None, 0, None) == -1
    assert b"k_sb" in lib.isi_last_error()
    with pytest.raises(_hip.HipLibraryError):
        from interactive_spectrogram_inpainting.priors import _ops
        _ops.rel_attention_decode(q, k, k, None, 4, 16, 15, 1, 1, 16, shared=True)


# ---------------------------------------------------------------- the loop

def _request(model, seed):
    """One request (batch 1) on `model`: condition, initial code, and a window mask that leaves a prefix of >= 8 positions."""
    F, T = model.shape
    g = torch.Generator().manual_seed(seed)
    init = torch.randint(0, 32, (1, F, T), generator=g)
    cond = None if model.self_conditional_model else torch.randint(0, 32, (1,) + tuple(model.condition_shape), generator=g)
    mask = _window_mask(F, T, slice(0, F), slice(1, 3) if T == 4 else slice(3, 6))
    S = model.target_transformer_sequence_length
    mseq = model.target_codemaps_helper.to_sequence(mask).reshape(-1, S)[0].numpy()
    assert int(np.flatnonzero(mseq)[0]) + model.target_start_symbol.shape[1] - 1 >= 8, "the prefill must run"
    return init, cond, mask, g


def _sample(model, N, uni, init, cond, mask, variations, kv=None, temperature=0.9, top_p=0.9):
    import sample as S
    if variations:
        return S.sample_model(model, _dev(), 1, list(model.shape), temperature=temperature, condition=cond,
                              class_conditioning=CLS, initial_code=init.clone(), mask=mask, top_p_sampling_p=top_p,
                              uniforms=uni, kv_cache_dtype=kv, num_variations=N)
    return S.sample_model(model, _dev(), N, list(model.shape), temperature=temperature,
                          condition=None if cond is None else cond.repeat(N, 1, 1), class_conditioning=CLS,
                          initial_code=init.repeat(N, 1, 1), mask=mask, top_p_sampling_p=top_p, uniforms=uni,
                          kv_cache_dtype=kv)


def _loop_equivalence(model, name, seed, kv=None):
    """num_variations=N returns the codes of the repeated batch, code for code (no allowance: a differing code fails).
    N = 1, 5, 32 as the issue sets them (the per-row kernel reading the one copy with batch stride 0) and N = 64, from where
    the loop runs the row-block kernel."""
    init, cond, mask, g = _request(model, seed)
    S = model.target_transformer_sequence_length
    for N in (1, 5, 32, 64):
        uni = torch.rand(S, N, generator=g)
        got = _sample(model, N, uni, init, cond, mask, True, kv)
        ref = _sample(model, N, uni, init, cond, mask, False, kv)
        assert got.shape == ref.shape == (N,) + tuple(model.shape)
        diff = int((got != ref).sum())
        print(f"variations {name} kv={kv} N={N}: {diff} of {int(mask.sum()) * N} sampled codes differ from the repeated batch")
        assert diff == 0, f"{name} N={N}: {diff} codes differ from the repeated batch"
        keep = ~mask.expand(N, -1, -1)
        assert torch.equal(got.cpu()[keep], init.expand(N, -1, -1)[keep]), "unmasked positions must keep initial_code"


def test_variations_equal_the_repeated_batch(golden_dir):
    """Test 2: top and bottom prior, plain cross-attention."""
    _, top, bottom = _models(golden_dir)
    _loop_equivalence(top, "top", 71)
    _loop_equivalence(bottom, "bottom", 72)


def test_variations_equal_the_repeated_batch_single_source(golden_dir):
    """Test 2, single-source priors: the table row is read with batch stride 0."""
    _loop_equivalence(_aligned_bottom(golden_dir), "aligned bottom", 73)
    _loop_equivalence(_identity_top(golden_dir), "identity top", 74)


def test_variations_equal_the_repeated_batch_bf16_caches(golden_dir):
    """Test 4: bf16 caches on both sides, same rule."""
    _, top, bottom = _models(golden_dir)
    _loop_equivalence(top, "top", 75, torch.bfloat16)
    _loop_equivalence(bottom, "bottom", 76, torch.bfloat16)


def test_variations_graph_replay_equals_direct_launches(golden_dir):
    from interactive_spectrogram_inpainting import _hip
    _, top, bottom = _models(golden_dir)
    for model, seed in ((top, 77), (bottom, 78)):
        init, cond, mask, g = _request(model, seed)
        uni = torch.rand(model.target_transformer_sequence_length, 5, generator=g)
        want = _sample(model, 5, uni, init, cond, mask, True)
        with _hip.knob("ISI_PRIOR_GRAPH", 0):
            assert torch.equal(_sample(model, 5, uni, init, cond, mask, True), want)
        assert torch.equal(_sample(model, 5, uni, init, cond, mask, True), want), "same uniforms, same maps"


def test_variations_differ_and_keep_unmasked_codes(golden_dir):
    """Test 3: eight variations at temperature 1 are not all equal; every row keeps the initial code outside the mask.
    Uniforms from `generator` when none are given; N beyond 256 runs in chunks."""
    import sample as S
    _, top, bottom = _models(golden_dir)
    for model, seed in ((top, 81), (bottom, 82)):
        init, cond, mask, g = _request(model, seed)
        out = S.sample_model(model, _dev(), 1, list(model.shape), temperature=1.0, condition=cond, class_conditioning=CLS,
                             initial_code=init.clone(), mask=mask, generator=torch.Generator().manual_seed(seed),
                             num_variations=8)
        assert out.shape == (8,) + tuple(model.shape) and int(out.min()) >= 0 and int(out.max()) < 32
        assert not bool((out == out[:1]).all()), "eight draws at temperature 1 came out identical"
        keep = ~mask.expand(8, -1, -1)
        assert torch.equal(out.cpu()[keep], init.expand(8, -1, -1)[keep])
    init, cond, mask, g = _request(top, 83)
    uni = torch.rand(top.target_transformer_sequence_length, 260, generator=g)
    big = _sample(top, 260, uni, init, cond, mask, True)
    assert big.shape == (260, 8, 4)
    assert torch.equal(big[256:], _sample(top, 4, uni[:, 256:], init, cond, mask, True))


def test_variations_default_untouched(golden_dir, monkeypatch):
    """Test 5: without num_variations the state handed to the library has memory_shared == 0 and a memory_kv with the batch
    dimension; with it, memory_shared == 1 and one copy."""
    import sample as S
    _, top, bottom = _models(golden_dir)
    seen = []

    class Recording(S.NativeSampler):
        def run(self, *a):
            seen.append(self)
            return super().run(*a)
    monkeypatch.setattr(S, "NativeSampler", Recording)
    init, cond, mask, g = _request(bottom, 91)
    N = 5
    uni = torch.rand(bottom.target_transformer_sequence_length, N, generator=g)
    L, d = len(bottom.transformer.decoder.layers), bottom.d_model
    _sample(bottom, N, uni, init, cond, mask, False)
    sm = seen[-1]
    assert sm.state.memory_shared == 0 and not sm.shared_memory
    assert tuple(sm.memory_kv.shape) == (L, sm.state.S_src, N, 2 * d)
    _sample(bottom, N, uni, init, cond, mask, True)
    sv = seen[-1]
    assert sv.state.memory_shared == 1 and tuple(sv.memory_kv.shape) == (L, sv.state.S_src, 1, 2 * d)
    assert tuple(sv.kv_cache.shape) == tuple(sm.kv_cache.shape)
    assert sv.memory_kv.numel() * N == sm.memory_kv.numel()


def test_ragged_plan_refuses_a_shared_memory(golden_dir):
    """Test 6a: memory_shared together with a ragged plan is refused by the library, by name."""
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    _, top, _ = _models(golden_dir)
    dev = _dev()
    B = 3
    init = torch.randint(0, 32, (1, 8, 4)).to(dev)
    clsd = {k: v.long().reshape(1, 1).to(dev) for k, v in CLS.items()}
    src, tgt = top.to_sequences(init, init, class_conditioning=clsd)
    memory, *_ = top.transformer.encoder(src.transpose(0, 1).contiguous(), mask='anticausal')
    x_seq = tgt.transpose(0, 1).repeat(1, B, 1).contiguous()
    codes = top.target_codemaps_helper.to_sequence(init).repeat(B, 1).contiguous()
    S = codes.shape[1]
    sm = NativeSampler(top, memory, x_seq, codes, [True] * S, torch.zeros(S, B), shared_memory=True)
    pos = np.minimum(np.arange(4)[:, None] + np.arange(B)[None, :], S - 1)
    n = sm.plan_rows(pos, np.zeros_like(pos))
    with pytest.raises(_hip.HipLibraryError, match="memory_shared"):
        sm.run_rows(0, n, 1.0, 0, 0.0)


def test_timerange_change_variations(golden_dir):
    """Test 7: four (top, bottom) pairs for one request; each equals the input outside the window, the tops are not all equal."""
    import inpainting
    z, top, bottom = _models(golden_dir)
    dev = _dev()
    cls = {k[5:]: torch.from_numpy(z[k])[:1].to(dev) for k in z.files if k.startswith("cls::")}
    g = torch.Generator().manual_seed(4)
    T_top, T_bot, start, N = 8, 16, 3, 4
    top_code = torch.randint(0, 32, (1, 8, T_top), generator=g).to(dev)
    bottom_code = torch.randint(0, 32, (1, 16, T_bot), generator=g).to(dev)
    mask = torch.zeros(1, 8, 4, dtype=torch.bool)
    mask[0, 2:6, 1:3] = True

    def run(layer, seed, m):
        return inpainting.timerange_change(top, bottom, top_code, bottom_code, m, layer, start, 1.0, cls, cls, dev,
                                           generator=torch.Generator().manual_seed(seed), top_p_sampling_p=0.9,
                                           num_variations=N)
    tops, bottoms = run("top", 1, mask)
    assert tops.shape == (N, 8, T_top) and bottoms.shape == (N, 16, T_bot)
    full_top = torch.zeros(1, 8, T_top, dtype=torch.bool, device=dev)
    full_top[..., start:start + 4] = mask.to(dev)
    full_bot = full_top.repeat_interleave(2, -2).repeat_interleave(2, -1)
    for n in range(N):
        assert torch.equal(tops[n:n + 1][~full_top], top_code[~full_top])
        assert torch.equal(bottoms[n:n + 1][~full_bot], bottom_code[~full_bot])
    assert int(tops.min()) >= 0 and int(tops.max()) < 32 and int(bottoms.min()) >= 0 and int(bottoms.max()) < 32
    assert not bool((tops == tops[:1]).all()), "four top variations came out identical"
    again = run("top", 1, mask)
    assert torch.equal(again[0], tops) and torch.equal(again[1], bottoms)
    mask_b = torch.zeros(1, 16, 8, dtype=torch.bool)
    mask_b[0, 4:9, 2:7] = True
    t2, b2 = run("bottom", 2, mask_b)
    assert torch.equal(t2, top_code.expand(N, -1, -1))
    fb = torch.zeros(1, 16, T_bot, dtype=torch.bool, device=dev)
    fb[..., 2 * start:2 * start + 8] = mask_b.to(dev)
    for n in range(N):
        assert torch.equal(b2[n:n + 1][~fb], bottom_code[~fb])
    assert not bool((b2 == b2[:1]).all())
