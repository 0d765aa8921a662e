"""Float64 NumPy specification of the optimizer step (plain Adam + global-norm clipping), shared by
tests/test_optimizer_host.py (which pins it to torch.optim.Adam + clip_grad_norm_ in float64) and
tests/test_optimizer_gpu.py (which holds the HIP kernels and torch's fp32 Adam to it)."""
import math

import numpy as np


def clip_coef(grads, max_norm):
    """(total_norm, coef) of `clip_grad_norm_(params, max_norm)`: coef = min(1, max_norm / (total_norm + 1e-6))."""
    total = math.sqrt(sum(float(np.sum(np.square(np.asarray(g, dtype=np.float64)))) for g in grads))
    if max_norm is None:
        return total, 1.0
    return total, min(1.0, float(max_norm) / (total + 1e-6))


def adam_step(p, g, m, v, lr, betas, eps, step, coef=1.0):
    """One Adam step of one tensor at step count `step` (>= 1); float64 in, float64 out: (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    g = g * coef
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** step)
    inv_sqrt_bc2 = 1.0 / math.sqrt(1.0 - b2 ** step)
    p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + eps)
    return p, m, v


def ulps(got, want):
    """max |got - want| in units of the fp32 spacing at `want` (got: fp32 array, want: float64 array)."""
    want = np.asarray(want, dtype=np.float64)
    spacing = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / spacing)) if want.size else 0.0


def _fma32(a, b, c):
    """fp32 fma of fp32 arrays: the product of two fp32 numbers is exact in float64; the sum is rounded to 53 bits and then
    to 24 (the double rounding moves a result by one fp32 spacing only on an exact tie of the second rounding)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam_step_all_fp32(p, g, m, v, lr, betas, eps, step, coef=1.0):
    """The update with an all-fp32 hyper block {b1, 1-b1, b2, 1-b2, eps, step_size, inv_sqrt_bc2} (each rounded once from
    double) and every operation in fp32, fused multiply-adds where the formula has them: the form the kernel does NOT use.
    Emulated on the host in IEEE fp32 so that its error against the float64 spec is on record beside the kernel's
    (tools/bench_optimizer.py, profiles/optimizer_step.json; DESIGN.md section 4.4 says what follows from it)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    h = [f(x) for x in (b1, 1.0 - b1, b2, 1.0 - b2, eps, lr / (1.0 - b1 ** step), 1.0 / math.sqrt(1.0 - b2 ** step))]
    gs = g * f(coef)
    m = _fma32(np.full_like(m, h[0]), m, h[1] * gs)
    v = _fma32(np.full_like(v, h[2]), v, (h[3] * gs) * gs)
    denom = _fma32(np.sqrt(v), np.full_like(v, h[6]), np.full_like(v, h[4]))
    p = _fma32(np.full_like(p, -h[5]), m / denom, p)
    return p, m, v


# ---------------------------------------------------------------------------------------------- the GPU accuracy problem
# Shared by tests/test_optimizer_gpu.py and tools/bench_optimizer.py (which records the figures the test quotes).
import torch  # noqa: E402

# (n, gradient 16-byte aligned inside the bucket?): the sizes of the issue -- 1 element, around the float4 width, around a
# wave / a workgroup, around one and two chunks of 2048, and 65 537 = 32 chunks + 1 element -- then 70 tiny tensors, which
# push the table past one launch's 64 entries.  Unaligned bucket offsets disagree with the parameter's own alignment mod 16
# (element-wise route); aligned ones take the float4 route with a tail.
LAYOUT = [(65537, True), (4097, True), (256, True), (4, True), (1, False), (3, False), (5, False), (255, False), (257, False),
          (4095, False)] + [((i % 7) + 1, False) for i in range(70)]
STEPS = 8
CLIP = {"off": None, "active": 20.0, "inactive": 1e6}      # the gradient norm of the set below is ~70 (asserted)


class Problem:
    """One optimizer over LAYOUT + two sliced parameters (4 bytes off 16-byte alignment) + one parameter without a gradient,
    in two param groups; gradients are views into one flat bucket."""

    def __init__(self, dev, ours: bool, **opt_kw):
        from interactive_spectrogram_inpainting.utils.training.optimizer import make_adam
        self.dev, self.ours = dev, ours
        sizes = [n for n, _ in LAYOUT] + [777, 300]
        self.sizes = sizes
        tensors = [torch.zeros(n, device=dev) for n, _ in LAYOUT]
        self.base_a, self.base_b = torch.zeros(1 + 777, device=dev), torch.zeros(1 + 300, device=dev)
        tensors += [self.base_a[1:], self.base_b[1:]] if ours else [torch.zeros(777, device=dev), torch.zeros(300, device=dev)]
        self.params = [torch.nn.Parameter(t) for t in tensors]
        self.idle = torch.nn.Parameter(torch.full((9,), 0.5, device=dev))         # never gets a gradient
        if ours:
            assert self.params[-2].data_ptr() % 16 == 4 and self.params[-1].data_ptr() % 16 == 4
        # bucket offsets
        offs, off = [], 0
        for n, aligned in LAYOUT:
            off = (off + 3) // 4 * 4 if aligned else off
            offs.append(off)
            off += n
        off = (off + 3) // 4 * 4 + 1            # sliced parameter A: gradient, moments and parameter all at residue 4 (head + tail)
        offs.append(off)
        off += 777
        off = (off + 3) // 4 * 4                # sliced parameter B: aligned gradient and moments, parameter at residue 4
        offs.append(off)
        off += 300
        self.bucket = torch.zeros(off, device=dev)
        self.grads = [self.bucket[o:o + n] for o, n in zip(offs, sizes)]
        if not ours:
            self.grads = [g.clone() for g in self.grads]
        groups = [{"params": self.params[0::2] + [self.idle]}, {"params": self.params[1::2], "lr": 3e-3, "betas": (0.85, 0.99)}]
        self.group_of = [i % 2 for i in range(len(self.params))]
        # the yardstick: torch's single-launch Adam, what make_adam gives the training scripts by default
        self.opt = make_adam(groups, lr=1e-3, device_hyper=True, **opt_kw) if ours else torch.optim.Adam(groups, lr=1e-3, fused=True)
        if ours:                                # moments of sliced parameter A share its residue mod 16
            self.m_a, self.v_a = torch.zeros(1 + 777, device=dev), torch.zeros(1 + 777, device=dev)
            self.opt.state[self.params[-2]].update(exp_avg=self.m_a[1:], exp_avg_sq=self.v_a[1:])

    def set_hyper(self, t):
        g0, g1 = self.opt.param_groups
        (g0["lr"], g0["betas"], _), (g1["lr"], g1["betas"], _) = group_hyper(t)
        return [(g["lr"], g["betas"], g["eps"]) for g in (g0, g1)]

    def load(self, P, G, M, V):
        with torch.no_grad():
            for i, q in enumerate(self.params):
                q.copy_(torch.from_numpy(P[i]))
                self.grads[i].copy_(torch.from_numpy(G[i]))
                q.grad = self.grads[i]
                st = self.opt.state[q]
                if M is not None and "exp_avg" in st:
                    st["exp_avg"].copy_(torch.from_numpy(M[i]))
                    st["exp_avg_sq"].copy_(torch.from_numpy(V[i]))

    def step(self, max_norm):
        if self.ours:
            self.opt.clip_grad_norm = max_norm
            self.opt.step()
            norm = self.opt.total_norm.clone() if max_norm is not None else None
        else:
            norm = torch.nn.utils.clip_grad_norm_(self.params, max_norm) if max_norm is not None else None
            self.opt.step()
        return norm

    def read(self):
        out = []
        for q in self.params:
            st = self.opt.state[q]
            out.append((q.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()))
        return out


_TRAJECTORIES = {}


def trajectory(mode):
    """Inputs and float64 outputs of the 8 steps (computed once per clip mode): every step starts from the fp32 rounding
    of the spec's previous outputs, so a bound on one step's error does not compound."""
    if mode in _TRAJECTORIES:
        return _TRAJECTORIES[mode]
    rng = np.random.default_rng(17)
    sizes = [n for n, _ in LAYOUT] + [777, 300]
    P = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    M = [np.zeros(n, np.float32) for n in sizes]
    V = [np.zeros(n, np.float32) for n in sizes]
    steps = []
    for t in range(1, STEPS + 1):
        G = [(rng.standard_normal(n) * 0.25).astype(np.float32) for n in sizes]
        groups = group_hyper(t)
        total, coef = clip_coef(G, CLIP[mode])
        out = [adam_step(P[i], G[i], M[i], V[i], *groups[i % 2][:2], groups[i % 2][2], t, coef) for i in range(len(sizes))]
        steps.append(dict(P=P, G=G, M=M, V=V, out=out, total=total, coef=coef))
        P, M, V = ([o[k].astype(np.float32) for o in out] for k in range(3))
    _TRAJECTORIES[mode] = steps
    return steps


def run_trajectory(problem, mode):
    """Runs the trajectory on one optimizer; returns (per-quantity max error in ulps, norm error in ulps, raw outputs)."""
    err = {"p": 0.0, "m": 0.0, "v": 0.0}
    norm_err, raw = 0.0, []
    for t, st in enumerate(trajectory(mode), start=1):
        problem.set_hyper(t)
        problem.load(st["P"], st["G"], st["M"] if t > 1 else None, st["V"] if t > 1 else None)
        norm = problem.step(CLIP[mode])
        got = problem.read()
        for (p, m, v), (sp, sm, sv) in zip(got, st["out"]):
            err["p"] = max(err["p"], ulps(p, sp))
            err["m"] = max(err["m"], ulps(m, sm))
            err["v"] = max(err["v"], ulps(v, sv))
        if norm is not None:
            norm_err = max(norm_err, ulps(norm.cpu().numpy(), np.float64(st["total"])))
            raw.append(norm.cpu().numpy().tobytes())
        raw.extend(a.tobytes() for trio in got for a in trio)
    return err, norm_err, raw


def group_hyper(t):
    """(lr, betas, eps) of the two param groups at step t of the trajectory."""
    return [(1e-3 * (1 + t), (0.95 - 0.01 * t, 0.999), 1e-8), (3e-3 / t, (0.85 + 0.01 * t, 0.99), 1e-8)]


def all_fp32_form_errors(mode):
    """Max error in ulps of `adam_step_all_fp32` against the spec over the trajectory (host only)."""
    err = {"p": 0.0, "m": 0.0, "v": 0.0}
    for t, st in enumerate(trajectory(mode), start=1):
        for i, out in enumerate(st["out"]):
            lr, betas, eps = group_hyper(t)[i % 2]
            got = adam_step_all_fp32(st["P"][i], st["G"][i], st["M"][i], st["V"][i], lr, betas, eps, t, st["coef"])
            for k, a, w in zip("pmv", got, out):
                err[k] = max(err[k], ulps(a, w))
    return err
