#!/usr/bin/env python3
"""What do random restarts of dead codes cost the replayed VQ-VAE training step?

Times the recorded (HIP-graph) training step of `train_vqvae.GraphedVQVAEStep` at the bench's shape (B = 64 of [2,128,512])
for three cases, each in a fresh child process, alternating A B C A B C ... so that drift of the box hits all alike:

  parent_plain   the plain model on a checkout of the parent commit (`--parent-tree DIR`, built there; omitted: not measured)
  plain          the plain model on this tree (its code path is unchanged: must equal parent_plain within the spread)
  restarts       VQVAE(restarts_usage_threshold=0.5) on this tree (one more small launch per quantiser, K D + K more floats
                 in each EMA-statistics message, the update kernel with restarts)

Writes profiles/codebook_restarts.json: per case the rounds' ms per step (device events around the replays), their median
and min..max = the box's run-to-run spread.  Records; gates nothing."""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent


def child(tree: pathlib.Path, threshold: float, replays: int, batch: int) -> None:
    sys.path.insert(0, str(tree / "interactive-spectrogram-inpainting_amd"))
    import torch
    import train_vqvae as T
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    kw = {} if threshold == 1.0 else {"restarts_usage_threshold": threshold}
    model = VQVAE(in_channel=2, **kw).to(dev).train()
    opt = make_adam(model.parameters(), lr=3e-4, capturable=True)
    crit = T.get_reconstruction_criterion("MSE")
    xs = [torch.randn(batch, 2, 128, 512, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(4)]
    for x in xs:
        x[:, 1].tanh_()
    step = T.GraphedVQVAEStep(model, crit, opt, xs[0], 0.25, None)
    for i in range(5):
        step(xs[i % 4])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(replays):
        o = step(xs[i % 4])
    b.record()
    torch.cuda.synchronize()
    step.finish()
    out = {"ms_per_step": a.elapsed_time(b) / replays, "segments": step.graphed.n_segments,
           "perplexity_t": float(o["perplexity_t"]), "perplexity_b": float(o["perplexity_b"])}
    for name in ("quantize_t", "quantize_b"):
        st = getattr(getattr(model, name), "restart_state", None)
        if st is not None:
            out[name + ".restart_state"] = st.tolist()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", type=pathlib.Path, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "codebook_restarts.json")
    ap.add_argument("--child", nargs=2, metavar=("TREE", "THRESHOLD"), default=None)
    args = ap.parse_args()
    if args.child:
        return child(pathlib.Path(args.child[0]), float(args.child[1]), args.replays, args.batch)
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    cases = []
    if args.parent_tree is not None:
        cases.append(("parent_plain", args.parent_tree.resolve(), 1.0))
    cases += [("plain", ROOT, 1.0), ("restarts", ROOT, 0.5)]
    runs = {name: [] for name, _, _ in cases}
    for r in range(args.rounds):
        for name, tree, thr in cases:
            p = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), "--child", str(tree), str(thr),
                                "--replays", str(args.replays), "--batch", str(args.batch)],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:      # nothing more is started on the GPU after a failed step
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{name}: child exited with {p.returncode}")
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            runs[name].append(res)
            print(f"round {r} {name}: {res['ms_per_step']:.4f} ms/step", flush=True)
    report = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "workload": f"replayed VQ-VAE training step (forward, backward, Adam), B={args.batch} of [2,128,512]",
              "unit": "ms per step (device events around the replays)",
              "method": f"cases alternate, {args.rounds} rounds of {args.replays} replays, a fresh process and recording "
                        "each; spread = min..max of a case's rounds",
              "parent_plain": None if args.parent_tree is not None else "not measured (no --parent-tree)"}
    for name, rs in runs.items():
        ms = [round(x["ms_per_step"], 4) for x in rs]
        report[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": ms,
                        "segments": rs[-1]["segments"], "perplexity_t": rs[-1]["perplexity_t"],
                        "perplexity_b": rs[-1]["perplexity_b"]}
        for k, v in rs[-1].items():
            if k.endswith("restart_state"):
                report[name][k] = v
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
