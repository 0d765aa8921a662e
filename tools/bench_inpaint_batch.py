#!/usr/bin/env python3
"""Batched inpainting requests against one request at a time, one JSON line.

BASELINE-size priors (random weights): the top prior [32,32] (self-conditional) and the bottom prior [64,64] over a [32,32]
top map, d_model 512, 6 + 8 layers.  N = 1 / 4 / 8 / 16 / 32 requests, each a 64-token window at its own random place
(top: 32 frequencies x 2 frames; bottom: 32 frequencies x 2 frames of the [64,64] map), temperature 1, top-p 0.8.
`sequential`: N `sample_model` calls of one row each; `batched`: one ragged call over the N rows.  Both in the same process,
alternated, synchronised before and after every timed call; median of 3 after one warm-up of each."""
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


def _masks(N, F, T, g):
    m = torch.zeros(N, F, T, dtype=torch.bool)
    for r in range(N):
        f0 = int(torch.randint(0, F - 32 + 1, (1,), generator=g))
        t0 = int(torch.randint(0, T // 2, (1,), generator=g)) * 2
        m[r, f0:f0 + 32, t0:t0 + 2] = True
    return m


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    import sample as S
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer, UpsamplingVQTransformer
    dev = torch.device("cuda", 0)
    out = {"unit": "s per N requests (64 masked tokens each); codes/s", "timing": "median of 3, sequential and batched alternated"}
    torch.manual_seed(2)
    top = SelfAttentiveVQTransformer(shape=[32, 32], condition_shape=[32, 32], self_conditional_model=True,
                                     add_mask_token_to_symbols=True, **FULL).to(dev).eval()
    torch.manual_seed(3)
    bottom = UpsamplingVQTransformer(shape=[64, 64], condition_shape=[32, 32], **FULL).to(dev).eval()
    for name, model, shape, cshape in (("bottom", bottom, [64, 64], [32, 32]), ("top", top, [32, 32], [32, 32])):
        for N in (1, 4, 8, 16, 32):
            g = torch.Generator().manual_seed(100 + N)
            cond = torch.randint(0, 512, [N] + cshape, generator=g)
            init = torch.randint(0, 512, [N] + shape, generator=g)
            mask = _masks(N, shape[0], shape[1], g)
            uni = torch.rand(model.target_transformer_sequence_length, N, generator=g)
            kw = dict(class_conditioning=CLS, top_p_sampling_p=0.8)

            def sequential():
                for r in range(N):
                    S.sample_model(model, dev, 1, shape, 1.0, condition=cond[r:r + 1], initial_code=init[r:r + 1],
                                   mask=mask[r:r + 1], uniforms=uni[:, r:r + 1], **kw)

            def batched():
                S.sample_model(model, dev, N, shape, 1.0, condition=cond, initial_code=init, mask=mask, uniforms=uni, **kw)

            sequential()
            batched()
            ts, tb = [], []
            for _ in range(3):
                ts.append(_timed(sequential))
                tb.append(_timed(batched))
            s, b = sorted(ts)[1], sorted(tb)[1]
            out[f"{name}_N{N}"] = {"sequential_s": round(s, 4), "batched_s": round(b, 4), "batched_over_sequential": round(b / s, 3),
                                   "codes_per_s_sequential": round(64 * N / s, 1), "codes_per_s_batched": round(64 * N / b, 1)}
            print(json.dumps({f"{name}_N{N}": out[f"{name}_N{N}"]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
