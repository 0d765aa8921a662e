#!/usr/bin/env python3
"""Optimizer step: torch's fused capturable Adam (+ clip_grad_norm_) against DeviceHyperAdam (csrc/optimizer.hip), on the
top prior's parameter set and the VQ-VAE's, with and without clipping, and the whole replayed top-prior training step under
each optimizer.  Candidates are timed INTERLEAVED (A B A B ...) in rounds, so a drift of the machine hits both; the spread
over the rounds of one candidate is reported next to the medians.  Also measures the accuracy figures the test suite quotes
(tests/test_optimizer_gpu.py).  Writes profiles/optimizer_step.json.

  python tools/bench_optimizer.py [--rounds 7] [--iters 50] [--steps 20] [--batch 8] [--out profiles/optimizer_step.json]
"""
import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402
from bench_prior import build  # noqa: E402
from interactive_spectrogram_inpainting.priors import _ops  # noqa: E402
from interactive_spectrogram_inpainting.utils.losses.prediction import LabelSmoothingLoss  # noqa: E402
from interactive_spectrogram_inpainting.utils.training.graphed_step import GraphedTrainingStep  # noqa: E402
from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam  # noqa: E402


def _note(msg):
    print(f"[bench_optimizer] {msg}", file=sys.stderr, flush=True)


def _timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def _interleaved(cands, rounds, iters):
    """cands: name -> callable.  Returns name -> {median_ms, min_ms, max_ms, rounds}."""
    for fn in cands.values():
        _timed(fn, max(3, iters // 5))          # warm-up
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(_timed(fn, iters))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "rounds": [round(x, 4) for x in v]} for k, v in times.items()}


def optimizer_only(shapes, dev, rounds, iters):
    """The bare optimizer step on a parameter set (gradients fixed, lr 0 so the values stay put)."""
    out = {"parameters": int(sum(torch.Size(s).numel() for s in shapes)), "tensors": len(shapes)}
    g = torch.Generator().manual_seed(0)
    for clip in (None, 1.0):
        sets = {}
        for which in ("torch_fused_capturable", "device_hyper"):
            ps = [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in shapes]
            for p in ps:
                p.grad = torch.randn(p.shape, generator=g).to(dev) * 0.01
            if which == "device_hyper":
                opt = make_adam(ps, lr=0.0, device_hyper=True, clip_grad_norm=clip)
                sets[which] = opt.step
            else:
                opt = make_adam(ps, lr=0.0, capturable=True)

                def step(ps=ps, opt=opt):
                    if clip is not None:
                        torch.nn.utils.clip_grad_norm_(ps, clip)
                    opt.step()
                sets[which] = step
        out["clip" if clip is not None else "no_clip"] = _interleaved(sets, rounds, iters)
        _note(f"bare optimizer, {out['parameters']} parameters, clip {clip}: done")
    # bytes a fused pass must move: 16 read + 12 written per element (+ 4 read for the norm); the same count is charged to
    # both candidates, so the two figures compare like the times (torch's clipping moves more than that)
    n = out["parameters"]
    for key, extra in (("no_clip", 0), ("clip", 4)):
        for which in out[key]:
            ms = out[key][which]["median_ms"]
            out[key][which]["GBps_of_required_bytes"] = round(n * (28 + extra) / ms / 1e6, 1)
    return out


def replayed_prior_step(dev, B, rounds, steps):
    """The whole top-prior training step replayed from HIP graphs under each optimizer (bench.py's step).  One recording
    is alive at a time (the library's packed-weight caches are shared by the process: a second model recorded beside the
    first invalidates what the first recording points to), so a round records candidate A, times it, drops it, then B."""
    g = torch.Generator().manual_seed(300)
    code = torch.randint(0, 512, (B, 32, 32), generator=g).to(dev)
    mask = (torch.rand(B, 32, 32, generator=g) < 0.5).to(dev)
    cls = {"pitch": torch.full((B, 1), 24, device=dev), "instrument_family_str": torch.zeros(B, 1, dtype=torch.long, device=dev)}
    crit = LabelSmoothingLoss(512, 0.1, dim=1)

    def one(which, clip):
        m = build(dev).train()
        if which == "device_hyper":
            opt = make_adam(m.parameters(), lr=3e-4, device_hyper=True, clip_grad_norm=clip)
        else:
            opt = make_adam(m.parameters(), lr=3e-4, capturable=True)

        def step(*_a):
            opt.zero_grad(set_to_none=True)
            src, tgt = m.to_sequences(code, condition=code, class_conditioning=cls, mask=mask)
            logits, _ = m(tgt, condition=src)
            loss = crit(m.to_time_frequency_map(logits, kind="target", permute_output_as_logits=True), code)
            loss.backward()
            if clip is not None and which != "device_hyper":
                torch.nn.utils.clip_grad_norm_(m.parameters(), clip)
            opt.step()
            return loss.detach()
        try:
            graphed = GraphedTrainingStep(step, (code, mask), warmup=2, index_limits={0: 512},
                                          range_params=[p for p in m.parameters() if p.dim() == 2],
                                          optimizers=[opt] if which == "device_hyper" else None)
            _timed(lambda: graphed(code, mask), 5)          # warm-up replays
            ms = _timed(lambda: graphed(code, mask), steps)
            assert torch.isfinite(graphed.loss).all()
            graphed.finish()
        finally:
            _ops.set_dropout_seed_base(None)
        return ms
    out = {}
    for clip in (None, 1.0):
        times = {"torch_fused_capturable": [], "device_hyper": []}
        for _ in range(rounds):
            for which in times:
                times[which].append(one(which, clip))
                _note(f"replayed step, clip {clip}, {which}: {times[which][-1]:.3f} ms")
        out["clip" if clip is not None else "no_clip"] = {
            k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "rounds": [round(x, 4) for x in v]} for k, v in times.items()}
    return out


def accuracy(dev):
    """The figures of tests/test_optimizer_gpu.py::test_adam_kernels_against_float64_spec (the problem and its runner
    are the test support module's, tests/optimizer_spec.py): max error against the float64 spec in fp32 ulps at the
    spec's value, for torch's fused Adam (+ clip_grad_norm_), for the kernel, and for the all-fp32 form of the update
    emulated on the host in IEEE fp32 (the form the kernel does not use: DESIGN.md section 4.4)."""
    import optimizer_spec as S
    out = {}
    for mode in ("off", "active", "inactive"):
        _note(f"accuracy, clipping {mode}")
        ref_err, ref_norm, _ = S.run_trajectory(S.Problem(dev, ours=False), mode)
        err, norm, _ = S.run_trajectory(S.Problem(dev, ours=True), mode)
        out[mode] = {"torch_fused": {**ref_err, "total_norm": ref_norm}, "device_hyper": {**err, "total_norm": norm},
                     "all_fp32_form_emulated": S.all_fp32_form_errors(mode)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--replay-rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--skip-replay", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "optimizer_step.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X; there is nothing to measure without it"
    dev = torch.device("cuda:0")
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "unit": "ms per step (device events)",
           "method": f"candidates alternate A B A B ...: {args.rounds} rounds of {args.iters} steps for the bare optimizer, "
                     f"{args.replay_rounds} rounds of {args.steps} replays (a fresh recording each) for the whole step; "
                     "spread = min..max of a candidate's rounds"}
    res["accuracy_ulps_vs_float64_spec"] = accuracy(dev)
    res["optimizer_only"] = {
        "top_prior": optimizer_only([tuple(p.shape) for p in build(dev).parameters()], dev, args.rounds, args.iters),
        "vqvae": optimizer_only([tuple(p.shape) for p in VQVAE(in_channel=2).parameters()], dev, args.rounds, args.iters)}
    if not args.skip_replay:
        res["replayed_top_prior_step"] = {"batch": args.batch, **replayed_prior_step(dev, args.batch, args.replay_rounds, args.steps)}
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
