"""Optimizer construction of the training scripts (train_vqvae.py:777, train_autoregressive_model.py:624-640:
`optim.Adam(model.parameters(), lr, eps)`).  Same update rule; on the GPU torch's single-launch ("fused")
implementation is asked for -- the default multi-tensor path issues ~40 launches of 40 us each for the prior's
19 M parameters (1.5 ms of a 50 ms step), the fused one a handful.

`make_adam(..., device_hyper=True)` returns `DeviceHyperAdam`: the same update by the library's own kernels
(csrc/optimizer.hip), with lr, the betas and the bias corrections read from a small block of device memory the host
rewrites before every step.  It exists for steps recorded into HIP graphs (utils/training/graphed_step.py): torch's
capturable Adam can read a tensor lr, but its betas are launch constants of the recording, and `CycleScheduler`
moves beta1 every step."""
from __future__ import annotations

import copy
import math
from typing import Iterable, List, Optional, Tuple

import numpy as np
import torch

# isi_adam_hyper (include/isi_hip.h): eight doubles; the kernel evaluates the update in double and rounds each result once
HYPER_DTYPE = np.dtype([(name, "<f8") for name in ("b1", "one_minus_b1", "b2", "one_minus_b2", "eps", "step_size",
                                                   "inv_sqrt_bc2", "reserved")])


def make_adam(params: Iterable[torch.nn.Parameter], lr: float, eps: float = 1e-8, device_hyper: bool = False, **kw):
    if device_hyper:
        return DeviceHyperAdam(params, lr=lr, eps=eps, **kw)
    params = list(params)
    on_gpu = bool(params) and all(p.is_cuda for p in params)
    if on_gpu and "fused" not in kw and "foreach" not in kw:
        try:
            return torch.optim.Adam(params, lr=lr, eps=eps, fused=True, **kw)
        except (RuntimeError, TypeError, ValueError):     # a torch build without the fused kernels
            pass
    return torch.optim.Adam(params, lr=lr, eps=eps, **kw)


def adam_hyper_row(lr: float, betas: Tuple[float, float], eps: float, step: int) -> tuple:
    """The isi_adam_hyper block of one param group at step count `step` (>= 1), as a HYPER_DTYPE record, computed in double."""
    b1, b2 = float(betas[0]), float(betas[1])
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    return (b1, 1.0 - b1, b2, 1.0 - b2, float(eps), float(lr) / bc1, 1.0 / math.sqrt(bc2), 0.0)


# ---- state_dict interchange with torch.optim.Adam.  torch keeps a `step` per parameter; this class keeps one count per
# param group (every parameter of a group that has a gradient is stepped together), so the conversion is: on the way out,
# the group's count is written into every parameter's state; on the way in, the counts of a group must agree.
def steps_from_adam_state(state_dict: dict) -> Tuple[dict, List[int]]:
    """(a copy of `state_dict` without the per-parameter `step` entries, the step count of every param group)."""
    out = {"state": {}, "param_groups": copy.deepcopy(state_dict["param_groups"])}
    steps: List[int] = []
    for gi, group in enumerate(out["param_groups"]):
        if group.get("amsgrad") or group.get("maximize") or group.get("weight_decay", 0) != 0:
            raise ValueError("DeviceHyperAdam is plain Adam: a state with amsgrad, maximize or weight_decay does not load")
        seen = set()
        for idx in group["params"]:
            st = state_dict["state"].get(idx)
            if st is None:
                continue
            if "max_exp_avg_sq" in st:
                raise ValueError("DeviceHyperAdam has no amsgrad state")
            step = st.get("step", 0)
            seen.add(int(round(float(step.item() if torch.is_tensor(step) else step))))
            out["state"][idx] = {k: v for k, v in st.items() if k != "step"}
        if len(seen) > 1:
            raise NotImplementedError(f"param group {gi} holds parameters at different step counts {sorted(seen)}: "
                                      "DeviceHyperAdam keeps one count per group")
        steps.append(seen.pop() if seen else 0)
        group.pop("step", None)
    return out, steps


def adam_state_with_steps(state_dict: dict, steps: List[int]) -> dict:
    """`state_dict` (without `step` entries) in torch.optim.Adam's form: every parameter state gets its group's count as
    the float32 CPU scalar torch's own Adam keeps."""
    out = {"state": {k: dict(v) for k, v in state_dict["state"].items()},
           "param_groups": copy.deepcopy(state_dict["param_groups"])}
    for group, step in zip(out["param_groups"], steps):
        group.pop("step", None)
        for idx in group["params"]:
            if idx in out["state"]:
                out["state"][idx]["step"] = torch.tensor(float(step), dtype=torch.float32)
    return out


def _same_dense_layout(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Both channels-last 4-D tensors of one shape: element i of the one's storage is element i of the other's."""
    return (a.dim() == 4 and a.shape == b.shape and a.stride() == b.stride()
            and a.is_contiguous(memory_format=torch.channels_last))


class DeviceHyperAdam(torch.optim.Optimizer):
    """Plain Adam (no amsgrad, no weight decay) on libisi_hip's kernels, every per-step hyper-parameter on the device.

    `step()` reads `lr` and `betas` from `param_groups` when it is called -- where `CycleScheduler`, `LambdaLR` and a
    hand edit write -- advances each group's step count, writes one isi_adam_hyper block per group into a pinned host slot
    and copies it to the device on the current stream, then launches.  While a step is being recorded
    (`graphed_step.recording()`) it only launches; the owner of the recording calls `upload_hyper()` in front of every
    replay (`GraphedTrainingStep(..., optimizers=[opt])`).  The pinned slots form a ring, each guarded by an event: the host
    may run ahead of the device by `ring_slots` steps before it waits.

    `clip_grad_norm` (constructor option / attribute; None = off): global-norm clipping fused into the step -- the norm of
    all gradients of the step is reduced in a fixed order, `coef = min(1, max_norm / (norm + 1e-6))` stays on the device and
    scales the gradient as the update reads it.  `.grad` itself is left UNSCALED (nothing reads it after the step);
    `total_norm` is the last norm as a device tensor.  A recording keeps the setting it was made with.

    Parameters and gradients: fp32, on one GPU, dense.  Sliced parameters and gradients that are views into a flat bucket
    are fine (csrc/optimizer.hip picks the access width per chunk).  A parameter whose `.grad` is None is skipped."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, amsgrad: bool = False, clip_grad_norm: Optional[float] = None,
                 ring_slots: int = 4, **ignored):
        if weight_decay != 0:
            raise ValueError("DeviceHyperAdam is the reference's plain Adam: weight_decay must be 0")
        if amsgrad or ignored.get("maximize"):
            raise ValueError("DeviceHyperAdam implements neither amsgrad nor maximize")
        for k in ignored:
            if k not in ("capturable", "fused", "foreach", "differentiable", "maximize", "decoupled_weight_decay"):
                raise TypeError(f"DeviceHyperAdam got an unexpected argument {k!r}")
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid lr / eps / betas")
        # (the keys torch.optim.Adam keeps in a param group: a state_dict of this class loads into it)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        device = None
        for group in self.param_groups:
            group["step"] = 0
            for p in group["params"]:
                if not p.is_cuda:
                    raise RuntimeError(f"DeviceHyperAdam: a parameter lives on {p.device}: this optimizer runs only on an "
                                       "MI355X (HIP kernels, no CPU fallback)")
                if p.dtype != torch.float32:
                    raise TypeError("DeviceHyperAdam: parameters must be float32")
                if device is not None and p.device != device:
                    raise RuntimeError("DeviceHyperAdam: all parameters must live on one GPU")
                device = p.device
        self.device = device
        self.clip_grad_norm = clip_grad_norm
        self.ring_slots = max(1, int(ring_slots))
        self._hyper = None          # device bytes of [n_groups] isi_adam_hyper; allocated with the ring at first use
        self._table_key = None
        self._table = None
        self._active_groups = None  # groups with a row in the table; None until a table has been built
        self._partials = None
        self._norm_coef = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self.param_groups[-1].setdefault("step", 0)
        self._hyper = None

    # ------------------------------------------------------------------ hyper-parameter block
    def _ensure_buffers(self) -> None:
        n = len(self.param_groups)
        if self._hyper is None or self._hyper.numel() != n * HYPER_DTYPE.itemsize:
            self._hyper = torch.zeros(n * HYPER_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
            self._ring = torch.zeros(self.ring_slots, n * HYPER_DTYPE.itemsize, dtype=torch.uint8).pin_memory()
            self._ring_np = self._ring.numpy().view(HYPER_DTYPE)          # [slots, n] records over the pinned bytes
            self._ring_events: List[Optional[torch.cuda.Event]] = [None] * self.ring_slots
            self._uploads = 0
        if self._norm_coef is None:
            self._norm_coef = torch.tensor([0.0, 1.0], dtype=torch.float32, device=self.device)

    def upload_hyper(self) -> None:
        """Advances the step count of every group that has a row in the current tensor table (a group none of whose
        parameters has a gradient is not stepped, like torch.optim.Adam's per-parameter counts; before any table exists:
        every group) and sends the hyper-parameters of that step to the device: an asynchronous copy from the next
        pinned slot on the current stream.  `step()` calls it itself outside a recording; a replayed step needs exactly
        one call in front of each replay."""
        self._ensure_buffers()
        slot = self._uploads % self.ring_slots
        ev = self._ring_events[slot]
        if ev is not None:
            ev.synchronize()        # the copy that last read this slot has run
        for gi, group in enumerate(self.param_groups):
            if self._active_groups is None or gi in self._active_groups:
                group["step"] += 1
            if group["step"] < 1:         # never stepped and no row in the table: the kernel does not read its block
                continue
            self._ring_np[slot, gi] = adam_hyper_row(group["lr"], group["betas"], group["eps"], group["step"])
        with torch.cuda.device(self.device):
            self._hyper.copy_(self._ring[slot], non_blocking=True)
            ev = ev or torch.cuda.Event()
            ev.record()
        self._ring_events[slot] = ev
        self._uploads += 1

    @property
    def total_norm(self) -> Optional[torch.Tensor]:
        """Gradient norm of the last clipped step (a 0-dim view of device memory the next step overwrites)."""
        return None if self._norm_coef is None else self._norm_coef[0]

    # ------------------------------------------------------------------ tensor table
    def _build_table(self, is_recording: bool):
        from ... import _hip
        rows = []
        for gi, group in enumerate(self.param_groups):
            if group["weight_decay"] != 0 or group["amsgrad"] or group["maximize"]:
                raise ValueError("DeviceHyperAdam is plain Adam: weight_decay / amsgrad / maximize cannot be switched on")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                    raise TypeError("DeviceHyperAdam: gradients must be dense float32 tensors of the parameter's shape and device")
                if not (p.is_contiguous() and g.is_contiguous()) and not _same_dense_layout(p, g):
                    raise ValueError("DeviceHyperAdam: a parameter and its gradient must be dense and laid out alike "
                                     "(contiguous views and slices are fine)")
                st = self.state[p]
                if "exp_avg" not in st:
                    if is_recording:
                        raise RuntimeError("DeviceHyperAdam: the moments of a parameter would be created inside a recording "
                                           "(and zeroed by every replay): run one eager step first")
                    if group["step"] > 0:
                        raise NotImplementedError("DeviceHyperAdam keeps one step count per param group: a parameter cannot "
                                                  "receive its first gradient after the group has been stepped")
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if not (all(t.is_contiguous() or _same_dense_layout(p, t) for t in (m, v)) and m.dtype == v.dtype == torch.float32
                        and m.device == v.device == p.device and m.numel() == v.numel() == p.numel()):
                    raise ValueError("DeviceHyperAdam: exp_avg / exp_avg_sq must be dense float32 laid out like the parameter")
                if p.numel():
                    rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), gi))
        key = tuple(rows)
        if key != self._table_key:
            arr = (_hip.isi_adam_tensor * max(1, len(rows)))()
            for i, r in enumerate(rows):
                arr[i] = _hip.isi_adam_tensor(*r, 0)
            self._table_key, self._table = key, arr
            self._active_groups = {r[5] for r in rows}
            self._n_chunks = int(_hip.lib().isi_adam_num_chunks(arr, len(rows))) if rows else 0
        return self._table, len(rows)

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        from ... import _hip
        from . import graphed_step
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        is_recording = graphed_step.recording()
        table, n = self._build_table(is_recording)
        if n == 0:                  # no parameter has a gradient: nothing is stepped, no count advances
            return loss
        self._ensure_buffers()
        if not is_recording:
            self.upload_hyper()
        lib = _hip.lib()
        with torch.cuda.device(self.device):
            stream = _hip.stream_ptr(self.device)
            coef = None
            if self.clip_grad_norm is not None:
                if self._partials is None or self._partials.numel() != self._n_chunks:
                    self._partials = torch.empty(self._n_chunks, dtype=torch.float32, device=self.device)
                _hip.check(lib.isi_grad_sumsq_f32(table, n, self._partials.data_ptr(), self._n_chunks, stream),
                           "isi_grad_sumsq_f32")
                _hip.check(lib.isi_grad_clip_coef_f32(self._partials.data_ptr(), self._n_chunks, float(self.clip_grad_norm),
                                                      self._norm_coef.data_ptr(), stream), "isi_grad_clip_coef_f32")
                coef = self._norm_coef.data_ptr() + 4
            _hip.check(lib.isi_adam_step_f32(table, n, self._hyper.data_ptr(), len(self.param_groups), coef, stream),
                       "isi_adam_step_f32")
        return loss

    # ------------------------------------------------------------------ state_dict <-> torch.optim.Adam
    def state_dict(self) -> dict:
        sd = super().state_dict()
        return adam_state_with_steps(sd, [g.get("step", 0) for g in sd["param_groups"]])

    def load_state_dict(self, state_dict: dict) -> None:
        stripped, steps = steps_from_adam_state(state_dict)
        super().load_state_dict(stripped)
        for group, step in zip(self.param_groups, steps):
            group["step"] = step
        self._table_key = None


def clip_and_step(parameters, optimizer, clip_grad_norm: Optional[float]) -> None:
    """`clip_grad_norm_` + `optimizer.step()` of the training loops; with a DeviceHyperAdam the clipping is the step's own
    (one fused pass, gradients left unscaled)."""
    if isinstance(optimizer, DeviceHyperAdam):
        optimizer.clip_grad_norm = clip_grad_norm
    elif clip_grad_norm is not None:
        torch.nn.utils.clip_grad_norm_(parameters, clip_grad_norm)
    optimizer.step()
