"""KV-cached sampling of priors whose decoder rows attend ONE source row: the aligned decoder layer
(`use_aligned_decoder=True`, row p sees the source token of its event p // Cd) and the identity memory mask
(`use_identity_memory_mask=True`, row p sees source row p).  The native loop runs their cross-attention as rows of a
table out_proj(V(memory)) (isi_prior_state.cross_out); these tests hold it to the full forward, which applies the masks."""
import numpy as np
import pytest
import torch

from test_prior_gpu import COMMON, FULL, _dev, _full_pass_sampling, _window_mask

pytestmark = pytest.mark.gpu

CLS = {"pitch": torch.tensor([20]), "instrument_family_str": torch.tensor([3])}


def _load(m, z, name):
    """The golden wrapper weights (transformer layers stay at their seeded init, as in test_prior_gpu._models); the aligned
    layers share the plain layers' parameter names, the identity-mask model has no cross-attention relative table."""
    own = m.state_dict()
    sd = {k[len(name) + 5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "::w::")}
    sd = {k: v for k, v in sd.items() if k in own and own[k].shape == v.shape}
    missing = m.load_state_dict(sd, strict=False)
    assert all(k.startswith("transformer.") for k in missing.missing_keys)
    return m.to(_dev()).eval()


def _aligned_bottom(golden_dir):
    from interactive_spectrogram_inpainting.priors.transformer import UpsamplingVQTransformer
    z = np.load(golden_dir / "prior_wrapper.npz")
    torch.manual_seed(5)
    return _load(UpsamplingVQTransformer(shape=[16, 8], condition_shape=[8, 4], use_aligned_decoder=True, **COMMON), z, "bottom")


def _identity_top(golden_dir):
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer
    z = np.load(golden_dir / "prior_wrapper.npz")
    torch.manual_seed(5)
    return _load(SelfAttentiveVQTransformer(shape=[8, 4], condition_shape=[8, 4], self_conditional_model=True,
                                            add_mask_token_to_symbols=True, use_identity_memory_mask=True, **COMMON), z, "top")


def _clsd(B):
    return {k: v.long().expand(B).reshape(B, 1).to(_dev()) for k, v in CLS.items()}


def _bottom_case(bottom, B, mask, seed, settings=((0.8, 0, 0.9), (0.0, 0, 1.0), (0.0, 5, 1.1)), knobs=()):
    """sample_model == the full-pass loop for each (top_p, top_k, temperature); unmasked codes kept; the same codes under
    every execution switch in `knobs`."""
    import sample as S
    from interactive_spectrogram_inpainting import _hip
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    cond = torch.randint(0, 32, (B, 8, 4), generator=g)
    init = torch.randint(0, 32, (B, 16, 8), generator=g)
    uni = torch.rand(bottom.target_transformer_sequence_length, B, generator=g)
    for top_p, top_k, temp in settings:
        run = lambda: S.sample_model(bottom, dev, B, [16, 8], temperature=temp, condition=cond, class_conditioning=CLS,
                                     initial_code=init.clone(), mask=mask, top_p_sampling_p=top_p, top_k_sampling_k=top_k,
                                     uniforms=uni)
        got = run()
        keep = ~mask.expand(B, -1, -1)
        assert torch.equal(got.cpu()[keep], init[keep]), "unmasked positions must keep initial_code"
        ref, n_masked = _full_pass_sampling(bottom, init.clone().to(dev), cond.to(dev), _clsd(B), mask.to(dev), uni,
                                            temp, top_k, top_p)
        assert n_masked == int(mask.sum())
        assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {n_masked * B} sampled codes differ"
        for name, value in knobs:
            with _hip.knob(name, value):
                assert torch.equal(run(), ref), f"{name}={value}"


def test_aligned_bottom_prior_sample_model_matches_full_pass_sampling(golden_dir):
    """Aligned bottom prior [16,8] at B = 2: everything masked, then a window (its prefix prefilled, its tail kept)."""
    bottom = _aligned_bottom(golden_dir)
    knobs = (("ISI_PRIOR_GRAPH", 0), ("ISI_PRIOR_GRAPH", 1), ("ISI_PRIOR_GRAPH", 3), ("ISI_PRIOR_GRAPH", 8),
             ("ISI_DECODE_NO_STAT_HANDOFF", 1))
    _bottom_case(bottom, 2, torch.ones(1, 16, 8, dtype=torch.bool), 31, knobs=knobs)
    _bottom_case(bottom, 2, _window_mask(16, 8, slice(3, 13), slice(2, 6)), 32, knobs=knobs[:1] + knobs[-1:])


def test_identity_memory_mask_top_prior_sample_model_matches_full_pass_sampling(golden_dir):
    """Self-conditional top prior [8,4] with the identity memory mask: row p attends memory row p only."""
    import sample as S
    from interactive_spectrogram_inpainting import _hip
    top = _identity_top(golden_dir)
    dev = _dev()
    for B, cols in ((2, slice(1, 3)), (1, slice(0, 4)), (5, slice(0, 4))):
        g = torch.Generator().manual_seed(40 + B)
        init = torch.randint(0, 32, (B, 8, 4), generator=g)
        mask = _window_mask(8, 4, slice(0, 8), cols)
        uni = torch.rand(top.target_transformer_sequence_length, B, generator=g)
        run = lambda: S.sample_model(top, dev, B, [8, 4], temperature=0.9, class_conditioning=CLS, initial_code=init.clone(),
                                     mask=mask, top_p_sampling_p=0.8, uniforms=uni)
        got = run()
        keep = ~mask.expand(B, -1, -1)
        assert torch.equal(got.cpu()[keep], init[keep])
        ref, _ = _full_pass_sampling(top, init.clone().to(dev), init.clone().to(dev), _clsd(B), mask.to(dev), uni, 0.9, 0, 0.8)
        assert torch.equal(got, ref), f"B={B}: {(got != ref).sum().item()} codes differ"
        for name, value in (("ISI_PRIOR_GRAPH", 0), ("ISI_PRIOR_GRAPH", 1), ("ISI_DECODE_NO_STAT_HANDOFF", 1)):
            with _hip.knob(name, value):
                assert torch.equal(run(), ref), (B, name, value)


def test_aligned_bottom_prior_batched_tiles_and_chunks(golden_dir):
    """B = 48 (beyond decode_mfma_rows: the stages run as matrix tiles, the statistics reach linear2's tile kernel) and
    B = 300 (two native calls of 256 + 44 rows) on a small window."""
    bottom = _aligned_bottom(golden_dir)
    _bottom_case(bottom, 48, _window_mask(16, 8, slice(4, 12), slice(3, 5)), 51, settings=((0.8, 0, 1.0),),
                 knobs=(("ISI_DECODE_NO_STAT_HANDOFF", 1),))
    _bottom_case(bottom, 300, _window_mask(16, 8, slice(6, 10), slice(4, 5)), 52, settings=((0.0, 0, 1.0),))


def test_aligned_bottom_prior_at_baseline_size_matches_full_pass_sampling():
    """Aligned [64,64] bottom prior (d_model 512, 6 + 8 layers, over a [32,32] top map) with a 64-token window against one
    full 4100-row pass per masked token."""
    import sample as S
    from interactive_spectrogram_inpainting.priors.transformer import UpsamplingVQTransformer
    torch.manual_seed(3)
    bottom = UpsamplingVQTransformer(shape=[64, 64], condition_shape=[32, 32], use_aligned_decoder=True,
                                     **FULL).to(_dev()).eval()
    dev = _dev()
    B = 1
    g = torch.Generator().manual_seed(23)
    cond = torch.randint(0, 512, (B, 32, 32), generator=g)
    init = torch.randint(0, 512, (B, 64, 64), generator=g)
    mask = _window_mask(64, 64, slice(10, 42), slice(34, 36))
    cls = {"pitch": torch.tensor([24]), "instrument_family_str": torch.tensor([0])}
    clsd = {k: v.long().expand(B).reshape(B, 1).to(dev) for k, v in cls.items()}
    uni = torch.rand(bottom.target_transformer_sequence_length, B, generator=g)
    got = S.sample_model(bottom, dev, B, [64, 64], temperature=1.0, condition=cond, class_conditioning=cls,
                         initial_code=init.clone(), mask=mask, top_p_sampling_p=0.8, uniforms=uni)
    keep = ~mask.expand(B, -1, -1)
    assert torch.equal(got.cpu()[keep], init[keep])
    ref, n_masked = _full_pass_sampling(bottom, init.clone().to(dev), cond.to(dev), clsd, mask.to(dev), uni, 1.0, 0, 0.8)
    assert n_masked == 64
    assert (got != ref).sum().item() <= 1, f"{(got != ref).sum().item()} of 64 sampled codes differ"


@pytest.mark.parametrize("kind", ["aligned", "identity"])
def test_single_source_cache_rows_equal_full_forward(golden_dir, kind):
    """The self-attention key / value cache of every layer after the first depends on the earlier layers' cross-attention:
    the rows the native loop (`run` over every position, nothing sampled) and the batched prefill (`prefill(S_t)`) leave there
    equal the keys / values the full masked forward forms, captured at each decoder layer's input."""
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    model = _aligned_bottom(golden_dir) if kind == "aligned" else _identity_top(golden_dir)
    dev = _dev()
    B = 3
    F, T = model.shape
    g = torch.Generator().manual_seed(61)
    init = torch.randint(0, 32, (B, F, T), generator=g).to(dev)
    cond = init if kind == "identity" else torch.randint(0, 32, (B,) + tuple(model.condition_shape), generator=g).to(dev)
    with torch.no_grad():
        src, tgt = model.to_sequences(init, cond, class_conditioning=_clsd(B))
        seen = {}
        hooks = [l.register_forward_pre_hook(lambda mod, args, i=i: seen.__setitem__(i, args[0].detach().clone()))
                 for i, l in enumerate(model.transformer.decoder.layers)]
        try:
            _, memory = model(tgt, src)
        finally:
            for h in hooks:
                h.remove()
        ref = [l.self_attn.project_kv(seen[i]) for i, l in enumerate(model.transformer.decoder.layers)]
        x_seq = tgt.transpose(0, 1).contiguous()
        S_t = x_seq.shape[0]
        codes = model.target_codemaps_helper.to_sequence(init).clone().contiguous()
        none = [False] * codes.shape[1]
        uni = torch.zeros(codes.shape[1], B, device=dev)
        looped = NativeSampler(model, memory, x_seq.clone(), codes.clone(), none, uni)
        assert looped.single_source and looped.memory_kv is None
        looped.run(0, S_t, 1.0, 0, 0.0)
        filled = NativeSampler(model, memory, x_seq.clone(), codes.clone(), none, uni)
        filled.prefill(S_t)
        torch.cuda.synchronize()
    for l in range(1, len(ref)):
        for name, s in (("run", looped), ("prefill", filled)):
            got, want = s.kv_cache[l], ref[l]
            err = ((got - want).abs().max() / want.abs().max()).item()
            assert err <= 1e-5, f"{kind} {name} layer {l}: {err:.2e}"


def test_flask_generate_with_aligned_bottom_prior(golden_dir):
    """One /generate and one /erase round trip of the server with an aligned bottom prior."""
    import json
    import flask_server
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    from GANsynth_pytorch.spectrograms_helper import SpectrogramsHelper
    from test_prior_gpu import _models
    _, top, _ = _models(golden_dir)
    bottom = _aligned_bottom(golden_dir)
    dev = _dev()

    class Enc:
        def __init__(self, classes):
            self.classes = list(classes)

        def transform(self, values):
            return np.array([self.classes.index(v) for v in values])

        def inverse_transform(self, indexes):
            return np.array([self.classes[int(i)] for i in indexes], dtype=object)
    encoders = {"pitch": Enc(range(24, 85)), "instrument_family_str": Enc([f"fam{i}" for i in range(11)])}
    torch.manual_seed(9)
    vq = VQVAE(in_channel=2, num_hidden_channels=32, n_res_block=1, num_residual_channels=8, embed_dim=16,
               num_embeddings=64, resolution_factors={"bottom": 4, "top": 2}).to(dev).eval()
    helper = SpectrogramsHelper(16000, 128, 32, 128).to(dev)
    app = flask_server.create_app(vq, top, bottom, encoders, dev, spectrograms_helper=helper, top_p=0.9, seed=0,
                                  spectrograms_upsampling_factor=2)
    c = app.test_client()
    r = c.get("/generate?pitch=60&instrument_family_str=fam3&temperature=1.0")
    assert r.status_code == 200
    body = r.get_json()
    b = np.array(body["bottom_code"])
    assert b.shape == (16, 8) and b.min() >= 0 and b.max() < 32
    # a top-layer inpainting request: the top window is resampled, the bottom map below it by the aligned prior
    mask = np.zeros((8, 4), dtype=bool)
    mask[1:5, 0:2] = True
    r2 = c.post("/timerange-change?layer=top&start_index_top=0&uniform_sampling=False&pitch=60&instrument_family_str=fam3"
                "&temperature=1.0", data=json.dumps(dict(body, mask=mask.tolist())))
    assert r2.status_code == 200
    b2 = r2.get_json()
    assert (np.array(body["top_code"])[~mask] == np.array(b2["top_code"])[~mask]).all()
    bc = np.array(b2["bottom_code"])
    assert bc.shape == (16, 8) and bc.min() >= 0 and bc.max() < 64     # (codes of the VQ-VAE's 64-entry codebook)
