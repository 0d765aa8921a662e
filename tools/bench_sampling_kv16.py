#!/usr/bin/env python3
"""Sampled codes/s of KV-cached sampling with fp32 against bf16 key/value caches (kv_cache_dtype), one JSON line and
profiles/sampling_kv16.json (or --out):
  - the baseline top prior ([32,32], self-conditional, d_model 512, 6 + 8 layers), full mask: 1024 codes per sequence;
  - the baseline bottom prior ([64,64] over a [32,32] top map) on a 128-token window at the END of the map (two frames, every
    frequency: positions 3840 .. 3967, the self-attention cache nearly full; the prefix is prefilled by one batched pass),
at B = 1 / 8 / 32 / 128, the two formats alternated in the same process on the same device.  Per row: codes/s of the whole
`sample_model` call, codes/s of the native loop alone (device time of NativeSampler.run between two events: no encoder, no
prefill), and the bytes of the two caches.  Random weights, temperature 1, top-p 0.8; median of 3 calls after one warm-up.
--f32-only leaves the keyword out altogether (the fp32 rows on a checkout that predates it)."""
import argparse
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
LOOP = {"events": [], "bytes": None}


def _instrument():
    """Device time of the native loop alone, and the cache sizes, read off NativeSampler.run."""
    from interactive_spectrogram_inpainting.priors._decode import NativeSampler
    orig = NativeSampler.run

    def run(self, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig(self, *a, **k)
        e1.record()
        LOOP["events"].append((e0, e1))
        nbytes = lambda t: 0 if t is None else t.numel() * t.element_size()
        LOOP["bytes"] = (nbytes(self.kv_cache), nbytes(self.memory_kv))

    NativeSampler.run = run


def _time(fn, n_codes):
    fn(0)
    torch.cuda.synchronize()
    ts, loops = [], []
    for rep in range(3):
        LOOP["events"].clear()
        t0 = time.perf_counter()
        fn(1 + rep)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        loops.append(sum(a.elapsed_time(b) for a, b in LOOP["events"]) * 1e-3)
    return {"codes_per_s": round(n_codes / sorted(ts)[1], 1), "loop_codes_per_s": round(n_codes / sorted(loops)[1], 1),
            "kv_cache_bytes": LOOP["bytes"][0], "memory_kv_bytes": LOOP["bytes"][1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--f32-only", action="store_true")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sampling_kv16.json"))
    args = ap.parse_args()
    import sample as S
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer, UpsamplingVQTransformer
    _instrument()
    dev = torch.device("cuda", 0)
    formats = [("f32", {})] if args.f32_only else [("f32", {"kv_cache_dtype": torch.float32}), ("bf16", {"kv_cache_dtype": torch.bfloat16})]
    out = {"unit": "sampled codes/s", "timing": "median of 3 calls after one warm-up; loop = device time of the native loop alone",
           "device": torch.cuda.get_device_name(0), "rows": {}}
    torch.manual_seed(2)
    top = SelfAttentiveVQTransformer(shape=[32, 32], condition_shape=[32, 32], self_conditional_model=True,
                                     add_mask_token_to_symbols=True, **FULL).to(dev).eval()
    for B in args.batches:
        for name, kw in formats:
            run = lambda seed: S.sample_model(top, dev, B, [32, 32], 1.0, class_conditioning=CLS, top_p_sampling_p=0.8,
                                              generator=torch.Generator().manual_seed(seed), **kw)
            out["rows"][f"top_B{B}_{name}"] = _time(run, 1024 * B)
            print(f"top_B{B}_{name}", out["rows"][f"top_B{B}_{name}"], flush=True)
    del top
    torch.cuda.empty_cache()
    torch.manual_seed(3)
    bottom = UpsamplingVQTransformer(shape=[64, 64], condition_shape=[32, 32], **FULL).to(dev).eval()
    mask = torch.zeros(1, 64, 64, dtype=torch.bool)
    mask[:, :, 60:62] = True
    for B in args.batches:
        g = torch.Generator().manual_seed(23)
        cond = torch.randint(0, 512, (B, 32, 32), generator=g)
        init = torch.randint(0, 512, (B, 64, 64), generator=g)
        for name, kw in formats:
            run = lambda seed: S.sample_model(bottom, dev, B, [64, 64], 1.0, condition=cond, class_conditioning=CLS,
                                              initial_code=init, mask=mask, top_p_sampling_p=0.8,
                                              generator=torch.Generator().manual_seed(seed), **kw)
            out["rows"][f"bottom_B{B}_{name}"] = _time(run, 128 * B)
            print(f"bottom_B{B}_{name}", out["rows"][f"bottom_B{B}_{name}"], flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
