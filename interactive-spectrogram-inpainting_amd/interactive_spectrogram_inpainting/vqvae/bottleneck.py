"""Vector-quantisation bottleneck on MI355X.

Drop-in for the reference's `vqvae/bottleneck.py:30-119`
(`QuantizedBottleneck`, `UnquantizedBottleneck`): same buffers (`embed [D,K]`,
`cluster_size [K]`, `embed_avg [D,K]`), same return tuple
`(quantize, diff, embed_ind, perplexity)`.  The L2 nearest-neighbour search runs
in `isi_vq_nearest_f32` (codebook resident in LDS, exact-fp32 matrix pipe,
lane-local arg-min) without materialising the [N,K] distance / one-hot matrices.
`QuantizedBottleneckWithRestarts` (`:122-166`) wraps an absent third-party package
in the reference; here it is the same EMA codebook whose dead codes -- EMA usage
below a threshold -- are redrawn from the current batch's encoder outputs inside
the update kernel, by a specification of this project's own ("EMA
codebook with random restarts"; tests/restarts_spec.py).
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import nn, Tensor

from .. import _hip
from . import _ops


class QuantizedBottleneck(nn.Module):
    cluster_size: Tensor

    def __init__(self, dim: int, n_embed: int, decay: float = 0.99, eps: float = 1e-5,
                 embeddings_initial_variance: float = 1,
                 corruption_weights: Optional[List[float]] = None):
        super().__init__()
        self.dim = dim
        self.n_embed = n_embed
        self.decay = decay
        self.eps = eps
        self.corruption_weights = corruption_weights
        self.embeddings_initial_variance = embeddings_initial_variance
        embed = torch.randn(dim, n_embed) * np.sqrt(self.embeddings_initial_variance)
        self.register_buffer('embed', embed)
        self.register_buffer('cluster_size', torch.zeros(n_embed))
        self.register_buffer('embed_avg', embed.clone())
        self._packed = None
        self._packed_key = None

    def packed(self):
        """(codes [K,D], e2 [K]) for the HIP kernels, cached per buffer version."""
        key = (_hip.version_of(self.embed), self.embed.data_ptr(), self.embed.device)
        if self._packed is None or self._packed_key != key:
            self._packed = _ops.pack_codebook(self.embed)
            self._packed_key = key
        return self._packed

    def forward(self, input: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """input [..., D] channels-last.  Train mode also corrupts the indices when
        `corruption_weights` is set and updates the codebook buffers (bottleneck.py:63-73,79-92)."""
        if self.training:
            from ._train import QuantizeTrainFunction
            return QuantizeTrainFunction.apply(self, input)
        codes, e2 = self.packed()
        return _ops.vq_nearest(input, codes, e2)

    def embed_code(self, embed_id: Tensor) -> Tensor:
        # range check on the host like F.embedding's (one device sync; skipped while a HIP graph is being captured)
        if embed_id.numel() and embed_id.is_cuda and not torch.cuda.is_current_stream_capturing() and \
                (int(embed_id.min()) < 0 or int(embed_id.max()) >= self.n_embed):
            raise IndexError("index out of range in self")  # same failure class as F.embedding
        codes, _ = self.packed()
        return _ops.embed_code(embed_id, codes)

    def embed_mix(self, embed_ids: Tensor, weights: Tensor) -> Tensor:
        """embed_ids int64 [M, ...], weights fp32 [M, ...] -> [..., D]: per cell the weighted sum of M codebook rows
        (`_ops.embed_mix`).  No range check on the host: a zero weight hides its id, and a non-zero weight over an id
        outside the codebook makes that cell NaN on the device."""
        codes, _ = self.packed()
        return _ops.embed_mix(embed_ids, weights, codes)

    def nearest_codes(self, z_nhwc: Tensor, m: int = 1, allowed_codes=None, allowed_map: Optional[Tensor] = None
                      ) -> Tuple[Tensor, Tensor]:
        """z_nhwc [B, H, W, D] -> (ids int64 [M, B, H, W], dist fp32 [M, B, H, W]): the `m` nearest codes of every cell by
        the bottleneck's own metric, nearest first, ties to the lower code (`_ops.vq_nearest_topm`).  `allowed_codes`: the
        palettes the search is restricted to, in any form `_ops.pack_palettes` takes (a bool row [K] as
        `sample.codes_in_use` returns it, a bool table [P, K], a list of index tensors) or an already packed word table;
        `allowed_map` [B, H, W] names each cell's palette (None: the first).  A palette with fewer than `m` codes leaves
        id -1 / distance +inf in the missing ranks.  The codebook is not updated, in any mode."""
        codes, e2 = self.packed()
        allowed = None
        if allowed_codes is not None:
            packed = (torch.is_tensor(allowed_codes) and allowed_codes.dtype == torch.int32 and allowed_codes.dim() == 2
                      and allowed_codes.shape[1] == (self.n_embed + 31) // 32)
            allowed = allowed_codes.to(z_nhwc.device) if packed else _ops.pack_palettes(allowed_codes, self.n_embed, z_nhwc.device)
        elif allowed_map is not None:
            raise ValueError("allowed_map selects rows of allowed_codes, which is not given")
        return _ops.vq_nearest_topm(z_nhwc, codes, e2, m, allowed, allowed_map)

    def distance_rows(self, z: Tensor) -> Tensor:
        """z [..., D] -> fp32 [..., K]: every vector's squared distance to every code, |z - E[k]|^2 -- the per-cell rows
        `CodeIndex.search_soft` compares stored codes with (`_ops.code_distance_rows`).  A vector that is codebook row `a`
        bit for bit gives row `a` of the code distance table bit for bit.  The codebook is not updated, in any mode."""
        codes, _ = self.packed()
        return _ops.code_distance_rows(z, codes)


class QuantizedBottleneckWithRestarts(QuantizedBottleneck):
    """EMA codebook with random restarts of dead codes (the reference's `bottleneck.py:122-166`, whose arithmetic sits in
    the absent `discretization` package: the behaviour is this project's own specification).

    Every training step, after the EMA update of `cluster_size` / `embed_avg`, a code whose `cluster_size` is below
    `restart_threshold` (vectors per step) becomes a row of the batch's pre-quantisation vectors, chosen by a
    counter-based hash of (`seed`, step, code index): `embed[:, k]` = that row exactly, `cluster_size[k]` = the threshold.
    `initialize`: the first step of a fresh module redraws every code.  The choice is made on the device from the
    `restart_state` buffer (int64 [4] = seed, step, restarts at the last step, restarts in total), so a step recorded
    into a HIP graph keeps drawing new rows on every replay.  The forward itself -- search, `diff`, perplexity -- uses the
    codebook from before the update and equals `QuantizedBottleneck`'s."""
    restart_state: Tensor

    def __init__(self, dim: int, n_embed: int, decay: float = 0.99, eps: float = 1e-5, restart_threshold: float = 1.,
                 initialize: bool = True, seed: int = 0, embeddings_initial_variance: float = 1,
                 corruption_weights: Optional[List[float]] = None):
        if corruption_weights is not None:      # the reference sets corruption_weights = None in this class (:129)
            warnings.warn("QuantizedBottleneckWithRestarts does not corrupt indices: corruption_weights is ignored")
        super().__init__(dim, n_embed, decay=decay, eps=eps, embeddings_initial_variance=embeddings_initial_variance,
                         corruption_weights=None)
        self.restart_threshold = float(restart_threshold)
        self.initialize = bool(initialize)
        seed = int(seed) % (1 << 64)
        self.register_buffer('restart_state',
                             torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed, 0, 0, 0], dtype=torch.int64))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key = prefix + 'restart_state'
        if key not in state_dict:
            # a checkpoint of the plain bottleneck: its codebook is trained, so `initialize` must not redraw it
            warnings.warn(f"{key} is missing from the state dict (a QuantizedBottleneck checkpoint): the restart step "
                          "starts at 1, the codebook is not re-initialised")
            state = self.restart_state.clone()
            state[1], state[2], state[3] = 1, 0, 0
            state_dict = dict(state_dict)
            state_dict[key] = state
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class UnquantizedBottleneck(QuantizedBottleneck):
    def forward(self, input):
        output = input
        diff = torch.zeros((1,), dtype=input.dtype, device=input.device)
        embed_ind = None
        code_assignation_perplexity = torch.as_tensor([np.inf], device=input.device)
        return output, diff, embed_ind, code_assignation_perplexity

    def embed_code(self, embed_ind):
        raise NotImplementedError

    def embed_mix(self, embed_ids, weights):
        raise NotImplementedError

    def nearest_codes(self, z_nhwc, m=1, allowed_codes=None, allowed_map=None):
        raise NotImplementedError

    def distance_rows(self, z):
        raise NotImplementedError
