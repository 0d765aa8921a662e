"""The opt-in bf16 key/value cache of KV-cached prior sampling (kv_cache_dtype=torch.bfloat16 / ISI_DECODE_KV=bf16):
the cached attention on bf16 rows (isi_rel_attention_decode_kv16_f32), the converting k|v store of every row kernel, and the
loop through NativeSampler, IncrementalDecoder and sample_model.  fp32 stays the default and is untouched."""
import contextlib
import math

import numpy as np
import pytest
import torch

from test_prior_gpu import TOL, _close, _dev, _models

pytestmark = pytest.mark.gpu

# bf16 operands: the bound test_rel_attention_bf16_mode accepts (of the reference's maximum), taken over
BF16_TOL = 2e-2


def _formula(q, k, v, rel, H, nk, q_pos, Cq, Ck, Ek):
    """float64 cached attention of one query row per (batch, head): key j reads table row q_pos // Cq - j // Ck + Ek - 1."""
    B, d = q.shape
    hd = d // H
    hq = q.view(B, H, hd).cpu().double()
    hk = k[:nk].float().view(nk, B, H, hd).permute(1, 2, 0, 3).cpu().double()
    hv = v[:nk].float().view(nk, B, H, hd).permute(1, 2, 0, 3).cpu().double()
    logit = torch.einsum("bhd,bhjd->bhj", hq, hk)
    if rel is not None:
        idx = (q_pos // Cq - torch.arange(nk) // Ck + Ek - 1).clamp(0, rel.shape[1] - 1)
        logit = logit + torch.einsum("bhd,hjd->bhj", hq, rel.cpu().double()[:, idx])
    return torch.einsum("bhj,bhjd->bhd", torch.softmax(logit / math.sqrt(hd), -1), hv).reshape(B, d).float()


def _check_case(q, k, v, rel, H, nk, q_pos, Cq, Ck, Ek, what):
    """Tests 1 and 2 of one case: the formula on the widened rows within TOL; the fp32 kernel on the widened rows within
    TOL; the one-workgroup and the two-launch form of the bf16 kernel bit for bit."""
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.priors import _ops
    assert k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16
    for r in (rel, None):
        got = _ops.rel_attention_decode(q, k, v, r, H, nk, q_pos, Cq, Ck, Ek)
        with _hip.knob("ISI_DECODE_ATTN_SEPARATE_SPLITS", 1):
            two = _ops.rel_attention_decode(q, k, v, r, H, nk, q_pos, Cq, Ck, Ek)
        assert torch.isfinite(got).all(), (what, nk, r is None)
        assert torch.equal(got, two), (what, nk, r is None, "one workgroup vs two launches")
        ref = _formula(q, k, v, r, H, nk, q_pos, Cq, Ck, Ek)
        _close(got, ref, TOL, f"{what} nk={nk} rel={r is not None}: formula")
        # the fp32 kernel never reads rows beyond nk either: hand it the widened rows (NaN rows included)
        f32 = _ops.rel_attention_decode(q, k.float(), v.float(), r, H, nk, q_pos, Cq, Ck, Ek)
        _close(got, f32, TOL, f"{what} nk={nk} rel={r is not None}: fp32 kernel on pre-rounded rows")


def test_kv16_attention_against_formula_and_fp32_kernel():
    """Tests 1 and 2 of the issue.  The bf16 kernel keeps 16-byte loads, so a lane holds eight elements of a row, a row has
    HD/8 lanes and twice the rows are in flight: a row's dot product keeps the fp32 kernel's tree, but the sums over KEYS
    (softmax denominator, p.v) run over twice the lane groups with half the keys each -- a different summation order is
    unavoidable with that grouping, so equality with the fp32 kernel on pre-rounded inputs is held to TOL (1e-4 of the
    maximum, no extra allowance: the rounding is in the inputs), and the bit-for-bit invariant pinned here is the one the
    fp32 kernel has: one-workgroup form == two-launch form (ISI_DECODE_ATTN_SEPARATE_SPLITS=1) of the new kernel."""
    dev = _dev()
    H, hd, S = 8, 64, 1024
    d = H * hd
    g = torch.Generator().manual_seed(31)
    rel = (torch.randn(H, 2 * S - 1, hd, generator=g) * 0.2).to(dev)
    for B in (32, 48):
        k = torch.randn(S, B, d, generator=g).bfloat16().to(dev)
        v = torch.randn(S, B, d, generator=g).bfloat16().to(dev)
        k[600:] = float("nan")                     # rows beyond the keys in use may hold anything
        v[600:] = float("nan")
        for nk in (1, 100, 144, 145, 300, 599, 600):
            q = torch.randn(B, d, generator=g).to(dev)
            _check_case(q, k, v, rel, H, nk, nk - 1, 1, 1, S, f"B={B}")
        k2 = torch.randn(S, B, d, generator=g).bfloat16().to(dev)     # the full cache
        v2 = torch.randn(S, B, d, generator=g).bfloat16().to(dev)
        q = torch.randn(B, d, generator=g).to(dev)
        for nk in (512, 513, 1024):
            _check_case(q, k2, v2, rel, H, nk, nk - 1, 1, 1, S, f"B={B} full cache")


@pytest.mark.parametrize("hd,H,B", [(16, 4, 1), (16, 4, 32), (32, 8, 1), (32, 8, 32), (64, 8, 1), (64, 8, 5)])
def test_kv16_attention_head_dims_and_split_counts(hd, H, B):
    """head_dim 16 / 32 / 64; batch 1 takes all 8 key splits and the combine launch, 5 sequences 8 as well, 32 two."""
    dev = _dev()
    S = 1024
    d = H * hd
    g = torch.Generator().manual_seed(7 + hd + B)
    rel = (torch.randn(H, 2 * S - 1, hd, generator=g) * 0.2).to(dev)
    k = torch.randn(S, B, d, generator=g).bfloat16().to(dev)
    v = torch.randn(S, B, d, generator=g).bfloat16().to(dev)
    k[700:] = float("nan")
    v[700:] = float("nan")
    for nk in (1, 100, 193, 321, 641, 700):
        q = torch.randn(B, d, generator=g).to(dev)
        _check_case(q, k, v, rel, H, nk, nk - 1, 1, 1, S, f"hd={hd} B={B}")


def test_kv16_attention_long_split_and_cross_geometry():
    """A long split (4100 keys of one sequence: 8 splits of 513 keys, beyond the rows a lane group holds in registers) and the
    bottom prior's cross-attention geometry (four query positions per event, one key per event: Cq = 4, Ck = 1)."""
    dev = _dev()
    H, hd = 8, 64
    d = H * hd
    g = torch.Generator().manual_seed(77)
    Sk = 4100
    k = torch.randn(Sk, 1, d, generator=g).bfloat16().to(dev)
    v = torch.randn(Sk, 1, d, generator=g).bfloat16().to(dev)
    rel = (torch.randn(H, 2 * Sk - 1, hd, generator=g) * 0.2).to(dev)
    for nk in (4100, 4099, 2000):
        q = torch.randn(1, d, generator=g).to(dev)
        _check_case(q, k, v, rel, H, nk, nk - 1, 1, 1, Sk, "long split")
    Ek = 1025
    relc = (torch.randn(H, 2 * Ek - 1, hd, generator=g) * 0.2).to(dev)
    for B in (1, 32):
        kc = torch.randn(Ek, B, d, generator=g).bfloat16().to(dev)
        vc = torch.randn(Ek, B, d, generator=g).bfloat16().to(dev)
        for q_pos in (0, 5, 2051, 4099):
            q = torch.randn(B, d, generator=g).to(dev)
            _check_case(q, kc, vc, relc, H, Ek, q_pos, 4, 1, Ek, f"cross B={B} q_pos={q_pos}")


def test_kv16_attention_refuses_mixed_dtypes():
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.priors import _ops
    dev = _dev()
    q = torch.randn(2, 64, device=dev)
    k = torch.randn(16, 2, 64, device=dev)
    for kk, vv in ((k.bfloat16(), k), (k, k.bfloat16()), (k.half(), k.half())):
        with pytest.raises(_hip.HipLibraryError):
            _ops.rel_attention_decode(q, kk, vv, None, 4, 16, 15, 1, 1, 16)


# ---------------------------------------------------------------- the loop

TIE_IN = (1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8)      # exactly between two bf16 values
TIE_BITS = (0x3F80, 0x3F82)                            # ... the even neighbour: 1.0 and 1 + 2^-6


def _tie_model(model):
    """Layer 0's key rows 0 and 1 become unit rows (zero bias): k[0], k[1] of every position are x[0], x[1] exactly, in every
    row kernel (one non-zero product per sum)."""
    sa = model.transformer.decoder.layers[0].self_attn
    d = model.d_model
    with torch.no_grad():
        sa.in_proj_weight[d:d + 2].zero_()
        sa.in_proj_weight[d, 0] = 1.0
        sa.in_proj_weight[d + 1, 1] = 1.0
        sa.in_proj_bias[d:d + 2].zero_()
    return model


def _sampler(model, B, kv_dtype, seed, mask=None, condition=None, tie=False):
    """A NativeSampler set up as sample_model does (all-zero mask by default: the loop steps without sampling)."""
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    F, T = model.shape
    init = torch.randint(0, 32, (B, F, T), generator=g).to(dev)
    if mask is None:
        mask = torch.zeros(1, F, T, dtype=torch.bool)
    mask = mask.to(dev)
    cls = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}
    clsd = {k: v.long().expand(B).reshape(B, 1).to(dev) for k, v in cls.items()}
    if model.self_conditional_model:
        condition = init
    elif condition is None:
        cF, cT = 8, 4
        condition = torch.randint(0, 32, (B, cF, cT), generator=g).to(dev)
    src, tgt = model.to_sequences(init, condition, class_conditioning=clsd, mask=mask)
    S = model.target_transformer_sequence_length
    code_seq = model.target_codemaps_helper.to_sequence(init).clone().contiguous()
    mask_seq = model.target_codemaps_helper.to_sequence(mask).reshape(-1, S).cpu().numpy()[0]
    memory, *_ = model.transformer.encoder(src.transpose(0, 1).contiguous(),
                                           mask='anticausal' if model.self_conditional_model else None)
    x_seq = tgt.transpose(0, 1).contiguous()
    if tie:
        x_seq[..., 0] = TIE_IN[0]
        x_seq[..., 1] = TIE_IN[1]
    uni = torch.rand(S, B, generator=g)
    return NativeSampler(model, memory, x_seq, code_seq, mask_seq, uni, kv_cache_dtype=kv_dtype), code_seq


def _ragged_positions(S_t, B):
    first = np.array([0, 3, 7, 1, 5, 2, 9, 4] * 4)[:B]
    pos = np.minimum(first[None, :] + np.arange(S_t)[:, None], S_t - 1).astype(np.int32)
    return pos, np.zeros_like(pos, dtype=np.uint8)


def _cache_pair(model, B, seed, ragged=False, tie=True):
    """(fp32 cache, bf16 cache) of the same teacher-forced run."""
    out = []
    for dt in (torch.float32, torch.bfloat16):
        sm, _ = _sampler(model, B, dt, seed, tie=tie)
        S_t = sm.x_seq.shape[0]
        if ragged:
            n = sm.plan_rows(*_ragged_positions(S_t, B))
            sm.run_rows(0, n, 1.0, 0, 0.0)
        else:
            sm.run(0, S_t, 1.0, 0, 0.0)
        torch.cuda.synchronize()
        assert sm.kv_cache.dtype == dt and sm.state.kv_format == (1 if dt is torch.bfloat16 else 0)
        out.append(sm.kv_cache.clone())
    return out


def _check_caches(f32, b16, what, worst):
    """Test 3: layer 0 bit for bit (its input rows are x_seq, which no precision touches), the two tie-to-even columns by
    their bits.  Test 4: deeper layers within BF16_TOL of the layer's maximum."""
    d2 = f32.shape[-1]
    d = d2 // 2
    assert torch.isfinite(b16.float()).all(), what
    assert torch.equal(b16[0], f32[0].bfloat16()), f"{what}: layer 0 is not the fp32 rows rounded to nearest-even"
    bits = b16[0].view(torch.int16)
    for c in (0, 1):
        seen = f32[0][..., c] != 0                       # (a ragged row never visits the slots before its first position)
        assert bool(seen.any()) and bool((f32[0][..., c][seen] == TIE_IN[c]).all()), f"{what}: the crafted key is not exact"
        assert bool((bits[..., c][seen] == TIE_BITS[c]).all()), f"{what}: tie {TIE_IN[c]!r} did not round to even"
    assert d > 2
    for l in range(1, f32.shape[0]):
        ref = f32[l].bfloat16().float()
        err = float((b16[l].float() - ref).abs().max() / ref.abs().max())
        print(f"kv16 cache {what} layer {l}: max err / max|ref| = {err:.3e}")
        worst.append(err)
        assert err < BF16_TOL, f"{what}: layer {l} differs by {err:.3e} of its maximum"


def test_kv16_converting_store_of_every_row_kernel(golden_dir):
    """Tests 3 and 4 of the issue on the golden top (3 layers, S_t = 33) and bottom (S_t = 129, Cq = 4) priors: one row
    (row_gemv1), 5 rows (row_gemvm), 5 rows on tiles (ISI_DECODE_MFMA_ROWS=1) and 20 rows (row_mfma32 + finish), direct
    launches and graph replay, and a ragged plan with rows at different positions (RAG instantiations).
    Observed maximum of test 4 over all of these (MI355X): 6.1e-3 of a layer's maximum, against the bound of 2e-2
    (profiles/sampling_kv16.json, "deeper_layer_max_err")."""
    from interactive_spectrogram_inpainting import _hip
    z, top, bottom = _models(golden_dir)
    worst = []
    for name, model in (("top", _tie_model(top)), ("bottom", _tie_model(bottom))):
        for graph in (0, None):
            tag = f"{name} graph={'default' if graph is None else graph}"
            ctx = _hip.knob("ISI_PRIOR_GRAPH", graph) if graph is not None else contextlib.nullcontext()
            with ctx:
                for B in (1, 5, 20):
                    _check_caches(*_cache_pair(model, B, 40 + B), f"{tag} B={B}", worst)
                with _hip.knob("ISI_DECODE_MFMA_ROWS", 1):
                    _check_caches(*_cache_pair(model, 5, 45), f"{tag} B=5 on tiles", worst)
                for B in (5, 20):
                    _check_caches(*_cache_pair(model, B, 50 + B, ragged=True), f"{tag} ragged B={B}", worst)
                with _hip.knob("ISI_DECODE_MFMA_ROWS", 1):
                    _check_caches(*_cache_pair(model, 5, 55, ragged=True), f"{tag} ragged B=5 on tiles", worst)
    print(f"kv16 deeper layers: observed maximum {max(worst):.3e}")


def test_kv16_incremental_decoder(golden_dir):
    """Test 5: IncrementalDecoder with bf16 caches against its fp32 rows and logits, within BF16_TOL; everything finite."""
    from interactive_spectrogram_inpainting.priors._decode import IncrementalDecoder
    z, top, bottom = _models(golden_dir)
    dev = _dev()
    cls = {k[5:]: torch.from_numpy(z[k]).to(dev) for k in z.files if k.startswith("cls::")}
    code = torch.from_numpy(z["top::code"]).to(dev)
    bcode = torch.from_numpy(z["bottom::code"]).to(dev)
    mask = torch.from_numpy(z["top::mask"]).to(dev)
    for name, m, (src, tgt) in (("top", top, top.to_sequences(code, code, class_conditioning=cls, mask=mask)),
                                ("bottom", bottom, bottom.to_sequences(bcode, code, class_conditioning=cls))):
        _, memory = m(tgt, src)
        ref = IncrementalDecoder(m, memory, tgt.shape[0])
        dec = IncrementalDecoder(m, memory, tgt.shape[0], kv_cache_dtype=torch.bfloat16)
        assert dec.cache[0].dtype == torch.bfloat16 and dec.memory_kv[0].dtype == torch.bfloat16
        x = tgt.transpose(0, 1).contiguous()
        for p in range(x.shape[0] - 1):
            want, got = ref.step(p, x[p]), dec.step(p, x[p])
            assert torch.isfinite(got).all()
            _close(got, want, BF16_TOL, f"{name} incremental row @ {p}")
            if p % 7 == 0:
                lg = dec.logits(got)
                assert torch.isfinite(lg).all()
                _close(lg, ref.logits(want), BF16_TOL, f"{name} incremental logits @ {p}")
        assert torch.equal(dec.cache[0], ref.cache[0].bfloat16()), f"{name}: layer 0 rows through the converting write"
    with pytest.raises(ValueError):
        IncrementalDecoder(top, memory, 1, kv_cache_dtype=torch.float16)


def _sample(model, B, uni, shape, kv, mask=None, init=None, condition=None, **kw):
    import sample as S
    cls = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}
    return S.sample_model(model, _dev(), B, shape, temperature=kw.pop("temperature", 1.0), class_conditioning=cls,
                          top_p_sampling_p=kw.pop("top_p", 0.9), uniforms=uni, mask=mask, condition=condition,
                          initial_code=init.clone() if init is not None else None, kv_cache_dtype=kv, **kw)


def _invariants(model, B, uni, shape, mask, init, condition=None, **kw):
    """Test 6's checks of one bf16 request; returns the map."""
    from interactive_spectrogram_inpainting import _hip
    bf = torch.bfloat16
    out = _sample(model, B, uni, shape, bf, mask, init, condition, **kw)
    assert out.shape == (B, *shape) and int(out.min()) >= 0 and int(out.max()) < 32
    if mask is not None:
        keep = ~mask.expand(B, -1, -1)
        assert torch.equal(out.cpu()[keep], init[keep]), "unmasked positions must keep initial_code"
    assert torch.equal(_sample(model, B, uni, shape, bf, mask, init, condition, **kw), out), "same uniforms, same map"
    with _hip.knob("ISI_PRIOR_GRAPH", 0):
        assert torch.equal(_sample(model, B, uni, shape, bf, mask, init, condition, **kw), out), "graph replay vs direct launches"
    with _hip.knob("ISI_DECODE_NO_STAT_HANDOFF", 1):
        assert torch.equal(_sample(model, B, uni, shape, bf, mask, init, condition, **kw), out), "statistics hand-off on / off"
    return out


def test_kv16_sampling_invariants(golden_dir):
    """Test 6: codes in range, unmasked positions kept, determinism, graph replay == direct launches, statistics hand-off
    on == off -- B = 1, 5, 20 and one ragged batch, top and bottom priors.  (Agreement with the fp32 run code for code is
    deliberately no criterion: after the first draw on the other side of a CDF boundary the contexts differ.)"""
    z, top, bottom = _models(golden_dir)
    g = torch.Generator().manual_seed(21)
    S_len = top.target_transformer_sequence_length
    mask = torch.zeros(1, 8, 4, dtype=torch.bool)
    mask[:, :, 1:3] = True
    for B in (1, 5, 20):
        uni = torch.rand(S_len, B, generator=g)
        init = torch.randint(0, 32, (B, 8, 4), generator=g)
        _invariants(top, B, uni, [8, 4], None, None)
        got = _invariants(top, B, uni, [8, 4], mask, init)
        ub = torch.rand(bottom.target_transformer_sequence_length, B, generator=g)
        _invariants(bottom, B, ub, [16, 8], None, None, condition=got)
    # a ragged batch: every row its own window and temperature
    B = 5
    rm = torch.zeros(B, 8, 4, dtype=torch.bool)
    for b in range(B):
        rm[b, :, b % 3:b % 3 + 1 + b % 2] = True
    uni = torch.rand(S_len, B, generator=g)
    init = torch.randint(0, 32, (B, 8, 4), generator=g)
    _invariants(top, B, uni, [8, 4], rm, init, temperature=[0.8, 0.9, 1.0, 1.1, 1.2])


def test_kv16_default_untouched(golden_dir, monkeypatch):
    """Test 7: no keyword == kv_cache_dtype=torch.float32, and the sampler's cache is fp32; ISI_DECODE_KV=bf16 == the keyword."""
    z, top, bottom = _models(golden_dir)
    monkeypatch.delenv("ISI_DECODE_KV", raising=False)
    g = torch.Generator().manual_seed(23)
    B = 5
    uni = torch.rand(top.target_transformer_sequence_length, B, generator=g)
    a = _sample(top, B, uni, [8, 4], None)
    assert torch.equal(a, _sample(top, B, uni, [8, 4], torch.float32))
    sm, _ = _sampler(top, B, torch.float32, 3)
    assert sm.kv_cache.dtype == torch.float32 and sm.memory_kv.dtype == torch.float32 and sm.state.kv_format == 0
    bf = _sample(top, B, uni, [8, 4], torch.bfloat16)
    monkeypatch.setenv("ISI_DECODE_KV", "bf16")
    assert torch.equal(_sample(top, B, uni, [8, 4], None), bf)
    monkeypatch.setenv("ISI_DECODE_KV", "f32")
    assert torch.equal(_sample(top, B, uni, [8, 4], None), a)


def test_kv16_prefill(golden_dir):
    """Test 8: a request with an unmasked prefix of >= 8 positions.  The bf16 cache rows of the prefix written by the batched
    causal pass agree with those written by single steps (prefill skipped) within BF16_TOL of each layer's maximum (GEMM
    and GEMV sum in different orders before the rounding: not bit for bit; observed 3.9e-4 / 2.7e-3 / 1.3e-3 for the three
    layers); the invariants of test 6 hold."""
    z, top, bottom = _models(golden_dir)
    mask = torch.zeros(1, 16, 8, dtype=torch.bool)
    mask[:, :, 3:6] = True                           # the first masked token is far behind position 8
    B = 5
    caches = []
    for prefill in (True, False):
        sm, _ = _sampler(bottom, B, torch.bfloat16, 61, mask=mask)
        first = int(np.flatnonzero(sm.mask_host)[0]) + sm.state.start_len - 1
        assert first >= 8
        if prefill:
            sm.prefill(first)
            sm.run(first, sm.x_seq.shape[0], 1.0, 0, 0.9)
        else:
            sm.run(0, sm.x_seq.shape[0], 1.0, 0, 0.9)
        torch.cuda.synchronize()
        caches.append(sm.kv_cache[:, :first].float().clone())
    for l in range(caches[0].shape[0]):
        err = float((caches[0][l] - caches[1][l]).abs().max() / caches[1][l].abs().max())
        print(f"kv16 prefill layer {l}: max err / max|ref| = {err:.3e}")
        assert torch.isfinite(caches[0][l]).all() and err < BF16_TOL, (l, err)
    g = torch.Generator().manual_seed(62)
    uni = torch.rand(bottom.target_transformer_sequence_length, B, generator=g)
    init = torch.randint(0, 32, (B, 16, 8), generator=g)
    cond = torch.randint(0, 32, (B, 8, 4), generator=g).to(_dev())
    _invariants(bottom, B, uni, [16, 8], mask, init, condition=cond)
