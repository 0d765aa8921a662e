"""GPU checks of the device-hyper Adam: the kernels of csrc/optimizer.hip against the float64 spec (tests/optimizer_spec.py)
with torch's own fp32 Adam on the same inputs as the yardstick, and recorded training steps that follow the host's
`param_groups` (utils/training/graphed_step.py, train_vqvae.py, train_autoregressive_model.py)."""
import argparse
import copy

import numpy as np
import pytest
import torch

import optimizer_spec as S

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- kernel against the spec
# Measured on an MI355X (profiles/optimizer_step.json, "accuracy_ulps_vs_float64_spec"): maximum error against the float64
# spec in fp32 ulps at the spec's value, torch 2.10 fused Adam + clip_grad_norm_ | this kernel:
#   clipping off       p 921.84   | 0.50      m 0.50      | 0.50       v 0.50 | 0.50
#   on and active      p 968.34   | 184.64    m 202946.74 | 77117.74   v 5.45 | 4.09     total_norm 1.41 | 0.41
#   on but inactive    p 921.84   | 0.50      m 0.50      | 0.50       v 0.50 | 0.50     total_norm 1.41 | 0.41
# (p: hundreds of ulps are elements where p - update cancels; active clipping: the spec scales g in double, both
# implementations round g * coef to fp32 first, which shows where the result cancels.)  REF_* are those reference errors:
REF_ULPS = {"off": {"p": 921.84, "m": 0.50, "v": 0.50}, "active": {"p": 968.34, "m": 202946.74, "v": 5.45},
            "inactive": {"p": 921.84, "m": 0.50, "v": 0.50}}        # on record only: the test measures torch again each run
REF_NORM_ULPS = 1.41
@pytest.mark.parametrize("mode", ["off", "active", "inactive"])
def test_adam_kernels_against_float64_spec(mode):
    """8 steps, lr and beta1 of both param groups changed every step, state re-seeded from the spec each step.  Per quantity
    (p, m, v, and total_norm where clipping is on) the kernel's maximum error may be at most twice the error of torch's own
    fp32 Adam (+ clip_grad_norm_) on the same GPU and inputs, with a floor of 1 ulp; two runs give identical bits; `.grad`
    is left unscaled; the parameter without a gradient is skipped."""
    dev = _dev()
    traj = S.trajectory(mode)
    assert 40.0 < traj[0]["total"] < 100.0
    assert all((s["coef"] < 1.0) == (mode == "active") for s in traj)
    ref_err, ref_norm_err, _ = S.run_trajectory(S.Problem(dev, ours=False), mode)
    ours = S.Problem(dev, ours=True)
    err, norm_err, raw = S.run_trajectory(ours, mode)
    print(f"optimizer accuracy [{mode}] torch: {ref_err} norm {ref_norm_err:.3f} | kernel: {err} norm {norm_err:.3f}")
    # the gradient is left as it was, the idle parameter untouched and stateless, the step counts are the host's
    assert torch.equal(ours.grads[0].cpu(), torch.from_numpy(traj[-1]["G"][0]))
    assert torch.equal(ours.idle.detach().cpu(), torch.full((9,), 0.5)) and "exp_avg" not in ours.opt.state[ours.idle]
    assert [g["step"] for g in ours.opt.param_groups] == [S.STEPS, S.STEPS]
    _, _, raw2 = S.run_trajectory(S.Problem(dev, ours=True), mode)
    assert raw == raw2, "two runs on equal inputs must give identical bits"
    for k in ("p", "m", "v"):
        assert err[k] <= max(2.0 * ref_err[k], 1.0), (k, err[k], ref_err[k])
    if mode != "off":
        assert norm_err <= max(2.0 * ref_norm_err, 1.0), (norm_err, ref_norm_err)


def test_non_finite_norm_propagates_and_hook_fires():
    """clip_grad_norm_'s default (error_if_nonfinite=False): a NaN gradient gives a NaN norm, a NaN coefficient and NaN
    parameters throughout, no exception; the
    library's global optimizer-step hook (packed-weight cache keys) fires for this class."""
    from interactive_spectrogram_inpainting import _hip
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    dev = _dev()
    p = torch.nn.Parameter(torch.ones(10, device=dev))
    opt = make_adam([p], lr=1e-2, device_hyper=True, clip_grad_norm=1.0)
    p.grad = torch.ones(10, device=dev)
    before = _hip.optimizer_steps()
    opt.step()
    assert _hip.optimizer_steps() == before + 1
    assert abs(float(opt.total_norm) - 10 ** 0.5) < 1e-5 and torch.isfinite(p).all()
    p.grad[3] = float("nan")
    opt.step()
    assert torch.isnan(opt.total_norm) and torch.isnan(p).all()


def test_step_counts_follow_the_gradients():
    """A step in which no parameter has a gradient advances nothing; a group none of whose parameters has a gradient is not
    stepped (torch.optim.Adam's per-parameter counts behave the same way)."""
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    dev = _dev()
    a, b = torch.nn.Parameter(torch.ones(5, device=dev)), torch.nn.Parameter(torch.ones(7, device=dev))
    opt = make_adam([{"params": [a]}, {"params": [b]}], lr=1e-2, device_hyper=True)
    opt.step()
    assert [g["step"] for g in opt.param_groups] == [0, 0]
    a.grad = torch.ones(5, device=dev)
    opt.step()
    opt.step()
    assert [g["step"] for g in opt.param_groups] == [2, 0]
    assert torch.equal(b.detach().cpu(), torch.ones(7)) and not torch.equal(a.detach().cpu(), torch.ones(5))
    # first step of Adam moves every element by lr (up to eps): 1 - 0.01, then again ~0.01
    assert abs(float(a[0]) - 0.98) < 1e-4


def test_state_dict_interchanges_with_torch_adam_on_the_gpu():
    """3 steps of torch.optim.Adam, its state_dict loaded into a DeviceHyperAdam, 2 more steps of each: the same parameters
    to fp32 rounding; and back: the DeviceHyperAdam's state_dict loads into a torch.optim.Adam that continues alike."""
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    init = [torch.randn(300, generator=g), torch.randn(17, 5, generator=g)]
    grads = [[torch.randn(300, generator=g).to(dev), torch.randn(17, 5, generator=g).to(dev)] for _ in range(7)]

    def fresh(**kw):
        ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
        return ps, make_adam(ps, lr=1e-2, **kw)

    def run(ps, opt, which):
        for k in which:
            for q, gr in zip(ps, grads[k]):
                q.grad = gr.clone()
            opt.step()
    ps_t, opt_t = fresh()
    run(ps_t, opt_t, range(3))
    ps_d, opt_d = fresh(device_hyper=True)
    with torch.no_grad():
        for a, b in zip(ps_d, ps_t):
            a.copy_(b)
    opt_d.load_state_dict(copy.deepcopy(opt_t.state_dict()))      # (state_dict() hands out the optimizer's own tensors)
    assert [g["step"] for g in opt_d.param_groups] == [3]
    run(ps_t, opt_t, range(3, 5))
    run(ps_d, opt_d, range(3, 5))
    for a, b in zip(ps_d, ps_t):
        assert float((a - b).abs().max()) <= 4e-7 * float(b.abs().max())
    sd = copy.deepcopy(opt_d.state_dict())
    assert all(float(st["step"]) == 5.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    ps_u, opt_u = fresh(foreach=True)
    with torch.no_grad():
        for a, b in zip(ps_u, ps_d):
            a.copy_(b)
    opt_u.load_state_dict(sd)
    run(ps_u, opt_u, range(5, 7))
    run(ps_t, opt_t, range(5, 7))
    for a, b in zip(ps_u, ps_t):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------- recorded steps
def _toy(dropout=0.0, seed=11, lr=1e-3, **opt_kw):
    """The toy prior of tests/test_prior_train_gpu.py::_toy_training_setup with a DeviceHyperAdam."""
    import test_prior_train_gpu as T
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer
    from interactive_spectrogram_inpainting.utils.losses.prediction import LabelSmoothingLoss
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    dev = _dev()
    torch.manual_seed(seed)
    model = SelfAttentiveVQTransformer(shape=[8, 4], condition_shape=[8, 4], self_conditional_model=True,
                                       add_mask_token_to_symbols=True, **T.COMMON).to(dev).train()
    for m in model.modules():
        if hasattr(m, "dropout") and isinstance(m.dropout, float):
            m.dropout = dropout
    g = torch.Generator().manual_seed(seed + 1)
    B = 4
    cls = {"instrument_family_str": torch.randint(0, 11, (B, 1), generator=g).to(dev),
           "pitch": torch.randint(0, 61, (B, 1), generator=g).to(dev)}
    batches = [(torch.randint(0, 32, (B, 8, 4), generator=g).to(dev), (torch.rand(B, 8, 4, generator=g) < 0.5).to(dev))
               for _ in range(7)]
    opt = make_adam(model.parameters(), lr=lr, device_hyper=True, **opt_kw)
    crit = LabelSmoothingLoss(32, 0.1, dim=1)

    def step(code, mask):
        opt.zero_grad(set_to_none=True)
        src, tgt = model.to_sequences(code, condition=code, class_conditioning=cls, mask=mask)
        logits, _ = model(tgt, condition=src)
        loss = crit(model.to_time_frequency_map(logits, kind="target", permute_output_as_logits=True), code)
        loss.backward()
        opt.step()
        return loss.detach()
    return model, opt, step, batches


def test_replays_follow_the_hosts_param_groups():
    """One recording: replayed with lr = 0 the parameters stay put; after a hand edit of param_groups' lr the same recording
    moves them."""
    from interactive_spectrogram_inpainting.priors import _ops
    from interactive_spectrogram_inpainting.utils.training.graphed_step import GraphedTrainingStep
    model, opt, step, batches = _toy(lr=0.0)
    graphed = GraphedTrainingStep(step, (batches[0][0].clone(), batches[0][1].clone()), warmup=1, index_limits={0: 32},
                                  optimizers=[opt])
    try:
        before = [p.detach().clone() for p in model.parameters()]
        graphed(*batches[1])
        torch.cuda.synchronize()
        assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
        for group in opt.param_groups:
            group["lr"] = 1e-2
        graphed(*batches[2])
        torch.cuda.synchronize()
        moved = sum(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
        assert moved > len(before) // 2, moved
        assert opt.param_groups[0]["step"] == 3        # one warm-up step, two replays
        graphed.finish()
    finally:
        _ops.set_dropout_seed_base(None)


@pytest.mark.parametrize("ring_slots,sync", [(4, True), (2, False)])
def test_graphed_step_with_cycle_scheduler_equals_eager(ring_slots, sync):
    """7 steps under a CycleScheduler (lr and beta1 move every step): one eager warm-up step and 6 replays against 7 eager
    steps of the same class from the same start, compared like tests/test_prior_train_gpu.py::
    test_graphed_training_step_equals_eager.  With a ring of 2 pinned slots and no synchronisation between the replays the
    host runs ahead of the device and has to wait for its slots."""
    from interactive_spectrogram_inpainting.priors import _ops
    from interactive_spectrogram_inpainting.utils.training.graphed_step import GraphedTrainingStep
    from interactive_spectrogram_inpainting.utils.training.scheduler import CycleScheduler
    model_e, opt_e, step_e, batches = _toy(clip_grad_norm=0.5)
    sched_e = CycleScheduler(opt_e, 5e-3, n_iter=6)
    losses_e = []
    for b in batches:
        losses_e.append(step_e(*b))
        sched_e.step()
    losses_e = [float(x) for x in losses_e]
    model_g, opt_g, step_g, _ = _toy(clip_grad_norm=0.5, ring_slots=ring_slots)
    sched_g = CycleScheduler(opt_g, 5e-3, n_iter=6)
    graphed = GraphedTrainingStep(step_g, (batches[0][0].clone(), batches[0][1].clone()), warmup=1, index_limits={0: 32},
                                  optimizers=[opt_g])
    sched_g.step()                               # (the warm-up step was step 1 of the schedule)
    try:
        losses_g = []
        for b in batches[1:]:
            loss = graphed(*b)
            sched_g.step()
            losses_g.append(float(loss) if sync else loss.clone())
        losses_g = [float(x) for x in losses_g]
        graphed.finish()
    finally:
        _ops.set_dropout_seed_base(None)
    assert opt_g.param_groups[0]["step"] == opt_e.param_groups[0]["step"] == 7
    for a, b in zip(losses_g, losses_e[1:]):
        assert abs(a - b) <= 2e-5 * abs(b), (losses_g, losses_e)
    for (name, pe), pg in zip(model_e.named_parameters(), model_g.parameters()):
        d = float((pe.detach() - pg.detach()).abs().max())
        assert d <= 2e-4 * max(1e-3, float(pe.abs().max())), (name, d)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(1e-12, float(b.double().abs().max()))


def test_train_vqvae_hip_graph_with_scheduler():
    """`train_vqvae.train(hip_graph=True, scheduler=CycleScheduler(...))` over 4 batches equals the eager `train` with the
    same optimizer class and schedule (tolerance of tests/test_train_gpu.py's graphed epoch test); a stock Adam still
    raises NotImplementedError."""
    import train_vqvae as T
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    from interactive_spectrogram_inpainting.utils.training.scheduler import CycleScheduler
    from interactive_spectrogram_inpainting.vqvae.vqvae import VQVAE
    dev = _dev()
    kw = dict(in_channel=2)
    data = T.SyntheticSpectrograms(16, shape=(2, 64, 128))
    crit = torch.nn.MSELoss()
    res = {}
    for graph in (False, True):
        torch.manual_seed(1)
        m = VQVAE(**kw).to(dev)
        opt = make_adam(m.parameters(), lr=1e-3, device_hyper=True)
        sched = CycleScheduler(opt, 2e-3, n_iter=4)
        loader = torch.utils.data.DataLoader(data, batch_size=4, shuffle=False, drop_last=True)
        means = T.train(0, loader, m, crit, opt, scheduler=sched, device=dev, clip_grad_norm=10.0, hip_graph=graph)
        assert opt.param_groups[0]["step"] == 4 and sched.count == 0
        res[graph] = (means, {k: v.clone() for k, v in m.state_dict().items()})
    for k in T.RunningMeans.NAMES:
        a, b = res[True][0][k], res[False][0][k]
        assert abs(a - b) <= 1e-4 * max(1e-6, abs(b)), (k, a, b)
    for k, v in res[False][1].items():
        assert _rel(res[True][1][k], v) < 1e-4, k
    torch.manual_seed(1)
    m = VQVAE(**kw).to(dev)
    stock = make_adam(m.parameters(), lr=1e-3, capturable=True)
    with pytest.raises(NotImplementedError):
        T.train(0, loader, m, crit, stock, scheduler=CycleScheduler(stock, 2e-3, n_iter=4), device=dev, hip_graph=True)


def test_run_model_hip_graph_equals_eager():
    """`run_model(..., hip_graph=True)` on a tiny top prior: 14 samples in batches of 4 (three replays and a ragged batch
    of 2, run eagerly) return the eager run's loss and accuracy sums, and nothing is left pending."""
    import test_prior_train_gpu as P
    import train_autoregressive_model as T
    from interactive_spectrogram_inpainting.priors.sequence_mask import BernoulliSequenceMask
    from interactive_spectrogram_inpainting.priors.transformer import SelfAttentiveVQTransformer
    from interactive_spectrogram_inpainting.utils.losses.prediction import LabelSmoothingLoss
    from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
    from interactive_spectrogram_inpainting.utils.training.scheduler import CycleScheduler

    class _SeededMask(BernoulliSequenceMask):
        """One mask per batch from a generator of its own (the recording's warm-up steps draw from torch's global one)."""
        gen = None

        def sample_mask(self, batch_size=1):
            self.gen = self.gen or torch.Generator().manual_seed(5)
            return torch.rand(batch_size, self.sequence_duration, generator=self.gen) < self.probability
    dev = _dev()
    data = T.SyntheticCodes(14, [8, 4], [16, 8], 32, {"instrument_family_str": 11, "pitch": 61}, seed=1)
    args = argparse.Namespace(hier="top")
    res = {}
    for graph in (False, True):
        torch.manual_seed(11)
        model = SelfAttentiveVQTransformer(shape=[8, 4], condition_shape=[8, 4], self_conditional_model=True,
                                           add_mask_token_to_symbols=True, **P.COMMON).to(dev)
        for mod in model.modules():
            if hasattr(mod, "dropout") and isinstance(mod.dropout, float):
                mod.dropout = 0.0
        loader = torch.utils.data.DataLoader(data, batch_size=4, shuffle=False)
        opt = make_adam(model.parameters(), lr=2e-3, device_hyper=True)
        sched = CycleScheduler(opt, 4e-3, n_iter=4)
        crit = LabelSmoothingLoss(32, 0.05, dim=1)
        sampler = _SeededMask(0.5, sequence_duration=model.source_transformer_sequence_length,
                              mask_token_index=model.mask_token_index)
        loss_sum, acc_sum, n = T.run_model(args, 0, loader, model, opt, sched, dev, crit, is_training=True,
                                           mask_sampler=sampler, clip_grad_norm=1.0, hip_graph=graph)
        assert n == 14 and opt.param_groups[0]["step"] == 4
        assert not model._index_guard._pending
        if graph:
            assert not model._graphed_train_step[1].graphed._pending
        res[graph] = (loss_sum, acc_sum, T.run_model.last_satisfied_constraints,
                      [p.detach().clone() for p in model.parameters()])
    for a, b in zip(res[True][:3], res[False][:3]):
        assert abs(a - b) <= 1e-4 * max(1e-6, abs(b)), (res[True][:3], res[False][:3])
    for a, b in zip(res[True][3], res[False][3]):
        assert _rel(a, b) < 1e-4
