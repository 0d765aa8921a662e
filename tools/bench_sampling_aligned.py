#!/usr/bin/env python3
"""Sampled codes/s of the single-source cross-attention mode against the all-rows form, one JSON line:
  - the baseline bottom prior ([64,64] over a [32,32] top map, d_model 512, 6 + 8 layers), plain vs use_aligned_decoder=True,
    at B = 1 / 8 / 32 / 128 on a fixed 64-token window (32 frequencies x 2 frames; the prefix is prefilled);
  - the baseline top prior ([32,32], self-conditional), plain vs use_identity_memory_mask=True, at B = 1 / 8, full mask.
Random weights, temperature 1, top-p 0.8; median of 3 calls after one warm-up call."""
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "interactive-spectrogram-inpainting_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

FULL = dict(n_class=512, channel=256, kernel_size=5, n_block=4, n_res_block=4, res_channel=256, d_model=512,
            embeddings_dim=32, positional_embeddings_dim=16, use_relative_transformer=True,
            predict_frequencies_first=True, conditional_model=True, class_conditioning_prepend_to_dummy_input=True,
            class_conditioning_num_classes_per_modality={"instrument_family_str": 11, "pitch": 61},
            class_conditioning_embedding_dim_per_modality={"instrument_family_str": 64, "pitch": 64})
CLS = {"pitch": torch.tensor([24]), "instrument_family_str": torch.tensor([0])}


def _time(fn, n_codes):
    fn(0)
    torch.cuda.synchronize()
    ts = []
    for rep in range(3):
        t0 = time.perf_counter()
        fn(1 + rep)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(n_codes / sorted(ts)[1], 1)


def main():
    import sample as S
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer, UpsamplingVQTransformer
    dev = torch.device("cuda", 0)
    out = {"unit": "sampled codes/s", "timing": "median of 3 calls after one warm-up"}
    mask = torch.zeros(1, 64, 64, dtype=torch.bool)
    mask[:, 10:42, 34:36] = True
    for aligned in (False, True):
        torch.manual_seed(3)
        m = UpsamplingVQTransformer(shape=[64, 64], condition_shape=[32, 32], use_aligned_decoder=aligned, **FULL).to(dev).eval()
        for B in (1, 8, 32, 128):
            g = torch.Generator().manual_seed(23)
            cond = torch.randint(0, 512, (B, 32, 32), generator=g)
            init = torch.randint(0, 512, (B, 64, 64), generator=g)
            run = lambda seed: S.sample_model(m, dev, B, [64, 64], 1.0, condition=cond, class_conditioning=CLS, initial_code=init,
                                              mask=mask, top_p_sampling_p=0.8, generator=torch.Generator().manual_seed(seed))
            out[f"bottom_{'aligned' if aligned else 'plain'}_B{B}"] = _time(run, 64 * B)
        del m
    for identity in (False, True):
        torch.manual_seed(2)
        m = SelfAttentiveVQTransformer(shape=[32, 32], condition_shape=[32, 32], self_conditional_model=True,
                                       add_mask_token_to_symbols=True, use_identity_memory_mask=identity, **FULL).to(dev).eval()
        for B in (1, 8):
            run = lambda seed: S.sample_model(m, dev, B, [32, 32], 1.0, class_conditioning=CLS, top_p_sampling_p=0.8,
                                              generator=torch.Generator().manual_seed(seed))
            out[f"top_{'identity' if identity else 'plain'}_B{B}"] = _time(run, 1024 * B)
        del m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
