#!/usr/bin/env python3
"""Per-cell mixtures of codes (csrc/code_mix.hip): kernel time of isi_embed_mix_f32 by device events (a replayed chain of
launches, warm, median of windows -- tools/bench_pitch.py's method) for the BOTTOM map of a batch of 64 flagship inputs
([2,128,512] -> 32 x 128 cells each, N = 262144, D = 64, K = 512) at M = 2 and M = 4 sources.  Beside each, in the same run:
  floor_us            the bytes the kernel must move -- the output stream N D 4 plus 12 M bytes per cell of ids and weights
                      (the 128 KB codebook stays in L2) -- over the HBM rate measured on this machine by the guide (6.29 TB/s,
                      not measured here)
  torch_expression    the same function as a torch expression, `(w[..., None] * E[ids]).sum(0)`: it materialises the
                      [M, N, D] gather
and a `morph_sweep` of 16 steps between two sounds of that size end to end (mixing both levels, one decode call).
The one condition: the kernel is not slower than the torch expression at either point (exit status 1 otherwise).  How
close the kernel comes to the floor is reported, not required.  Writes profiles/code_mix.json.

  python tools/bench_code_mix.py [--rounds 9] [--out profiles/code_mix.json]
"""
import argparse
import ctypes as C
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402
from bench_pitch import _chain  # noqa: E402
from bench_resample import HBM_MEASURED_BPS, _median, _note  # noqa: E402
from interactive_spectrogram_inpainting import _hip  # noqa: E402

B, HB, WB, D, K = 64, 32, 128, 64, 512
SWEEP_STEPS = 16


def torch_expression(ids, w, E):
    return (w[..., None] * E[ids]).sum(0)


def kernel_cases(dev, rounds):
    lib = _hip.lib()
    g = torch.Generator().manual_seed(0)
    E = torch.randn(K, D, generator=g).to(dev)
    N = B * HB * WB
    out_cases = []
    for M in (2, 4):
        ids = torch.randint(0, K, (M, N), generator=g).to(dev)
        w = torch.rand(M, N, generator=g)
        w = (w / w.sum(0)).to(dev)
        out = torch.empty(N, D, device=dev)

        def launch():
            _hip.check(lib.isi_embed_mix_f32(ids.data_ptr(), N, w.data_ptr(), N, E.data_ptr(), out.data_ptr(), D, N, M, D, K,
                                             C.c_void_p(_hip.stream_ptr(dev))), "isi_embed_mix_f32")
        t = _chain(launch, rounds)
        nbytes = N * D * 4 + 12 * M * N
        want = torch_expression(ids, w, E)
        launch()
        torch.cuda.synchronize()
        case = {"M": M, "N": N, "D": D, "K": K, "kernel": t, "bytes": nbytes,
                "floor_us": round(nbytes / HBM_MEASURED_BPS * 1e6, 3),
                "max_abs_diff_to_torch_expression": float((want - out).abs().max())}
        del want
        case["time_over_floor"] = round(t["median_us"] / case["floor_us"], 2)
        case["achieved_TB_per_s"] = round(nbytes / (t["median_us"] * 1e-6) / 1e12, 3)
        case["torch_expression"] = _median(lambda: torch_expression(ids, w, E), rounds)
        case["torch_expression_over_kernel"] = round(case["torch_expression"]["median_us"] / t["median_us"], 2)
        case["kernel_not_slower_than_torch_expression"] = t["median_us"] <= case["torch_expression"]["median_us"]
        out_cases.append(case)
        _note(json.dumps(case))
    return out_cases


def sweep(dev, rounds):
    import inpainting
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    torch.manual_seed(0)
    m = VQVAE(in_channel=2).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    a, b = ((torch.randint(0, K, (1, HB // 2, WB // 2), generator=g).to(dev), torch.randint(0, K, (1, HB, WB), generator=g).to(dev))
            for _ in range(2))
    t = _median(lambda: inpainting.morph_sweep(m, a, b, SWEEP_STEPS), rounds)
    t["decode_code_of_16_codemaps"] = _median(
        lambda: m.decode_code(a[0].expand(SWEEP_STEPS, -1, -1), a[1].expand(SWEEP_STEPS, -1, -1)), rounds)
    t["steps"] = SWEEP_STEPS
    t["what"] = ("inpainting.morph_sweep between two [2,128,512] sounds, public call: host-side weights, range check "
                 "(one sync), two mix launches, one decode of 16 spectrograms")
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "code_mix.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "unit": "microseconds per launch / call (device events around a window of back-to-back work, warm)",
           "floors": {"source": "HBM rate of the MI355X guide, not measured here", "hbm_bytes_per_s": HBM_MEASURED_BPS}}
    res["embed_mix_bottom_map_B64"] = kernel_cases(dev, args.rounds)
    res["morph_sweep"] = sweep(dev, args.rounds)
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    if not all(c["kernel_not_slower_than_torch_expression"] for c in res["embed_mix_bottom_map_B64"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
