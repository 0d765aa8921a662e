"""Query-by-example search of the code database on MI355X: "the stored sounds most like this one".

`extract_code.extract` writes the database, `LMDBDataset` reads it item by item on the host; a `CodeIndex` holds all of its
codemaps on the device (uint16, [N, F, T] per layer) with the items' class attributes, and compares a query codemap with
every stored one in one launch per layer (csrc/code_search.hip).  The metric is this project's own (DESIGN.md section 6c;
specification tests/code_search_spec.py): with the layer's codebook E [K, D],

    T[a][b]    = sum_d (E[a][d] - E[b][d])^2
    dist(q, x) = sum_c w[c] T[q[c]][x[c]]                cells with q[c] outside [0, K) -- the priors' mask token -- count nothing

and a two-layer distance is alpha dist_top + beta dist_bottom.  The bits of an item's distance depend on the query, the
weights, the item and the table only, so equal sounds stay tied and a ranking never flickers: results are ordered by
(distance ascending, item index ascending).  `search_shifted` answers the fragment question -- "which stored sound contains
something like this window, wherever it sits in time" -- with the same metric at every offset that fits
(csrc/code_shift_search.hip, specification tests/code_shift_search_spec.py).  No CPU path: the index, the VQ-VAE and the
queries must live on the GPU."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _hip

MAX_QUERIES = 64          # isi_code_search_f32: 1 <= Q <= 64 per launch
SHIFT_BUDGET_BYTES = 1 << 30      # search_shifted / distances_shifted: workspace + dist [Q, S, N] of one group of queries


def _as_codes(codes, name: str, n_embed: int) -> torch.Tensor:
    """[N, F, T] integer maps with every code in [0, n_embed) -> uint16 (ValueError otherwise)."""
    codes = torch.as_tensor(codes)
    if codes.dim() != 3 or codes.dtype.is_floating_point or codes.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"{name}: expected integer codemaps [N, F, T], got {codes.dtype} {tuple(codes.shape)}")
    if codes.numel() == 0:
        raise ValueError(f"{name}: no codemaps to index ({tuple(codes.shape)})")
    if codes.dtype != torch.uint16:
        lo, hi = int(codes.min()), int(codes.max())
        if lo < 0 or hi >= n_embed:
            raise ValueError(f"{name}: codes must lie in [0, {n_embed}), found {lo if lo < 0 else hi}")
        return codes.to(torch.int64).to(torch.uint16)
    signed = codes.view(torch.int16)                  # (no widened copy: a database of this type is gigabytes)
    lo, hi = int(signed.min()), int(signed.max())
    if lo < 0:                                        # bit patterns >= 2^15
        hi = 65536 + int(torch.where(signed < 0, signed, torch.full_like(signed, -32768)).max())
    if hi >= n_embed:
        raise ValueError(f"{name}: codes must lie in [0, {n_embed}), found {hi}")
    return codes


class CodeIndex:
    """The code database on the device.  Build with `from_arrays` or `from_dataset`."""

    def __init__(self, top: torch.Tensor, bottom: Optional[torch.Tensor], attributes: Mapping[str, torch.Tensor], vqvae,
                 label_encoders_per_modality: Optional[Mapping[str, object]] = None):
        self.top, self.bottom = top, bottom
        self.attributes = OrderedDict(attributes)
        self.vqvae = vqvae
        self.label_encoders = dict(label_encoders_per_modality or {})
        self.device = top.device
        self.top_shape = tuple(top.shape[1:])
        self.bottom_shape = tuple(bottom.shape[1:]) if bottom is not None else None
        self._tables = {}
        self._workspace = None
        self._derived = {}
        if 'pitch' in self.attributes:      # `sample_from_database`'s derived attributes, from the DECODED pitch
            pitch = self._decoded_long('pitch')
            self._derived = {'pitch_class': pitch % 12, 'octave': pitch // 12}

    # ---- construction
    @classmethod
    def from_arrays(cls, top, bottom, attributes: Mapping[str, torch.Tensor], vqvae, device,
                    label_encoders_per_modality: Optional[Mapping[str, object]] = None) -> "CodeIndex":
        """top [N, F_t, T_t], bottom [N, F_b, T_b] or None, attributes {name: encoded class index [N]} (as the database
        stores them).  ValueError for a code outside [0, n_embed) of its layer, or for counts that disagree."""
        device = torch.device(device)
        top = _as_codes(top, "top", int(vqvae.n_embed_t))
        if bottom is not None:
            bottom = _as_codes(bottom, "bottom", int(vqvae.n_embed_b))
            if bottom.shape[0] != top.shape[0]:
                raise ValueError(f"top holds {top.shape[0]} items, bottom {bottom.shape[0]}")
        attrs = OrderedDict()
        for name, values in attributes.items():
            values = torch.as_tensor(values).reshape(-1)
            if values.numel() != top.shape[0] or values.dtype.is_floating_point:
                raise ValueError(f"attribute {name}: expected {top.shape[0]} encoded class indices, got "
                                 f"{values.dtype} {tuple(values.shape)}")
            attrs[name] = values.to(device=device, dtype=torch.int64)
        return cls(top.to(device).contiguous(), None if bottom is None else bottom.to(device).contiguous(), attrs, vqvae,
                   label_encoders_per_modality)

    @classmethod
    def from_dataset(cls, codes_dataset: Sequence, vqvae, device,
                     label_encoders_per_modality: Optional[Mapping[str, object]] = None) -> "CodeIndex":
        """One pass over the items (top [F_t, T_t], bottom [F_b, T_b], {class name: tensor [1]}) of an `LMDBDataset` or of
        any sequence of its items.  ValueError for ragged shapes or a code outside [0, n_embed)."""
        n = len(codes_dataset)
        if n == 0:
            raise ValueError("the code database is empty")
        if label_encoders_per_modality is None:
            label_encoders_per_modality = getattr(codes_dataset, 'label_encoders', None) or None
        limits = (int(vqvae.n_embed_t), int(vqvae.n_embed_b))
        maps, attrs = None, None
        for i in range(n):
            top, bottom, encoded = codes_dataset[i]
            item = [np.asarray(torch.as_tensor(top)), np.asarray(torch.as_tensor(bottom))]
            if maps is None:
                maps = [np.empty((n,) + m.shape, np.uint16) for m in item]
                attrs = OrderedDict((name, np.empty(n, np.int64)) for name in encoded)
            for layer, (m, store, limit) in enumerate(zip(item, maps, limits)):
                if m.ndim != 2 or m.shape != store.shape[1:]:
                    raise ValueError(f"item {i}: {('top', 'bottom')[layer]} codemap {m.shape} differs from item 0's "
                                     f"{store.shape[1:]} (an index holds maps of one duration)")
                if m.dtype.kind not in 'iu' or m.min() < 0 or m.max() >= limit:
                    raise ValueError(f"item {i}: {('top', 'bottom')[layer]} codes must be integers in [0, {limit})")
                store[i] = m
            if set(encoded) != set(attrs):
                raise ValueError(f"item {i}: attributes {sorted(encoded)} differ from item 0's {sorted(attrs)}")
            for name, value in encoded.items():
                attrs[name][i] = int(torch.as_tensor(value).reshape(-1)[0])
        return cls.from_arrays(torch.from_numpy(maps[0]), torch.from_numpy(maps[1]),
                               {name: torch.from_numpy(v) for name, v in attrs.items()}, vqvae, device,
                               label_encoders_per_modality)

    # ---- items
    def __len__(self) -> int:
        return self.top.shape[0]

    def _check_item(self, i) -> int:
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(f"item {i} of an index of {len(self)}")
        return i % len(self)

    def __getitem__(self, i):
        """(top [F_t, T_t] int64, bottom [F_b, T_b] int64 or None, {class name: tensor [1]}), like a dataset item."""
        i = self._check_item(i)
        widen = lambda m: m[i].view(torch.int16).to(torch.int64).bitwise_and(0xFFFF)      # noqa: E731
        return (widen(self.top), None if self.bottom is None else widen(self.bottom),
                OrderedDict((name, values[i:i + 1]) for name, values in self.attributes.items()))

    def decoded_attributes(self, i) -> dict:
        """The attributes `sample_from_database` reports for an item: decoded classes, and `pitch_class` / `octave`."""
        i = self._check_item(i)
        out = {}
        for name, values in self.attributes.items():
            enc = int(values[i])
            out[name] = self.label_encoders[name].inverse_transform([enc])[0] if name in self.label_encoders else enc
        if 'pitch' in out:
            out['pitch_class'] = int(out['pitch']) % 12
            out['octave'] = int(out['pitch']) // 12
        return out

    def _decoded_long(self, name: str) -> torch.Tensor:
        values = self.attributes[name]
        if name not in self.label_encoders:
            return values
        uniq, inverse = torch.unique(values, return_inverse=True)
        decoded = [int(v) for v in self.label_encoders[name].inverse_transform(uniq.tolist())]
        return torch.tensor(decoded, dtype=torch.int64, device=values.device)[inverse]

    def allowed(self, attribute_constraints: Optional[Mapping[str, object]] = None,
                exclude: Optional[Sequence[int]] = None) -> Optional[torch.Tensor]:
        """uint8 [N] on the index's device: 1 where an item meets every constraint -- `sample_from_database`'s equality on
        the decoded attributes, `pitch_class` and `octave` derived from the decoded pitch -- and is not in `exclude`.
        None when nothing is constrained."""
        if not attribute_constraints and (exclude is None or len(exclude) == 0):
            return None
        ok = torch.ones(len(self), dtype=torch.bool, device=self.device)
        for name, wanted in (attribute_constraints or {}).items():
            if name in self._derived:
                try:
                    ok &= self._derived[name] == int(wanted)
                except (TypeError, ValueError):
                    ok[:] = False
            elif name in self.attributes:
                try:
                    enc = int(self.label_encoders[name].transform([wanted])[0]) if name in self.label_encoders else int(wanted)
                except (ValueError, KeyError, IndexError, TypeError):      # a value the encoder has never seen: no item has it
                    ok[:] = False
                else:
                    ok &= self.attributes[name] == enc
            else:
                ok[:] = False
        if exclude is not None and len(exclude):
            ok[torch.as_tensor([self._check_item(i) for i in exclude], dtype=torch.int64, device=self.device)] = False
        return ok.to(torch.uint8)

    # ---- tables
    def table(self, layer: str) -> torch.Tensor:
        """The layer's code distance table [K, K] fp32, rebuilt when the codebook buffer changes."""
        quantizer = self.vqvae.quantize_t if layer == 'top' else self.vqvae.quantize_b
        embed = quantizer.embed
        _hip.require_gpu(embed, f"quantize_{layer[0]}.embed")
        if embed.device != self.device:
            raise _hip.HipLibraryError(f"the VQ-VAE lives on {embed.device}, the index on {self.device}")
        key = (_hip.version_of(embed), embed.data_ptr(), embed.device)
        cached = self._tables.get(layer)
        if cached is None or cached[0] != key:
            codebook = embed.detach().t().contiguous()                  # [K, D]
            K, D = codebook.shape
            table = torch.empty(K, K, dtype=torch.float32, device=self.device)
            _hip.check(_hip.lib().isi_code_distance_table_f32(codebook.data_ptr(), table.data_ptr(), K, D,
                                                              C.c_void_p(_hip.stream_ptr(self.device))),
                       "isi_code_distance_table_f32")
            cached = (key, table)
            self._tables[layer] = cached
        return cached[1]

    # ---- search
    def _checked(self, layer: str, code, mask, window: bool = False):
        """(code [Q, F, T], mask or None, single) of one layer, shapes checked against the stored maps (ValueError).
        window: the query may be narrower than the stored maps, [Q, F, W] with 1 <= W <= T."""
        stored = self.top if layer == 'top' else self.bottom
        if stored is None:
            raise ValueError(f"{layer}_code given, but the index holds no {layer} maps")
        shape = tuple(stored.shape[1:])
        code = torch.as_tensor(code)
        if window:
            if code.dim() not in (2, 3) or code.shape[-2] != shape[0] or not 1 <= code.shape[-1] <= shape[1] \
                    or code.dtype.is_floating_point:
                raise ValueError(f"{layer}_code: expected integer windows [{shape[0]}, W] (or [Q, ...]) with 1 <= W <= "
                                 f"{shape[1]}, got {code.dtype} {tuple(code.shape)}")
            shape = (shape[0], int(code.shape[-1]))
        if code.dim() not in (2, 3) or tuple(code.shape[-2:]) != shape or code.dtype.is_floating_point:
            raise ValueError(f"{layer}_code: expected integer codemaps [{shape[0]}, {shape[1]}] (or [Q, ...]) like the "
                             f"stored ones, got {code.dtype} {tuple(code.shape)}")
        single = code.dim() == 2 or code.shape[0] == 1
        code = code.reshape(-1, *shape)
        Q = code.shape[0]
        if not 1 <= Q <= MAX_QUERIES:
            raise ValueError(f"{layer}_code: {Q} queries, a search takes 1..{MAX_QUERIES}")
        if mask is not None:
            mask = torch.as_tensor(mask)
            if mask.dtype != torch.bool or mask.dim() not in (2, 3) or tuple(mask.shape[-2:]) != shape \
                    or (mask.dim() == 3 and mask.shape[0] not in (1, Q)):
                raise ValueError(f"mask_{layer}: expected bool [{shape[0]}, {shape[1]}] (or [Q, ...]), got "
                                 f"{mask.dtype} {tuple(mask.shape)}")
        return code, mask, single

    def _query(self, layer: str, code: torch.Tensor, mask: Optional[torch.Tensor], weight: float):
        """(query uint16 [Q, C], weights fp32 [Q, C] or None) of one checked layer, on the device."""
        stored = self.top if layer == 'top' else self.bottom
        if not code.is_cuda or (mask is not None and not mask.is_cuda) or not stored.is_cuda:
            raise _hip.HipLibraryError(f"{layer}_code / mask_{layer} / the index live on "
                                       f"{code.device} / {None if mask is None else mask.device} / {stored.device}: this "
                                       "package computes only on an MI355X (HIP kernels, no CPU fallback)")
        Q, shape = code.shape[0], tuple(code.shape[1:])
        K = int(self.vqvae.n_embed_t if layer == 'top' else self.vqvae.n_embed_b)
        code = code.to(self.device, torch.int64)
        query = torch.where((code < 0) | (code > K), K, code).to(torch.uint16).reshape(Q, -1).contiguous()
        weights = None
        if mask is not None or float(weight) != 1.0:
            keep = torch.ones(Q, *shape, dtype=torch.bool, device=self.device) if mask is None \
                else ~mask.to(self.device).reshape(-1, *shape).expand(Q, *shape)
            weights = (keep.to(torch.float32) * float(weight)).reshape(Q, -1).contiguous()
        return query, weights

    def distances(self, top_code=None, bottom_code=None, *, mask_top=None, mask_bottom=None,
                  layer_weights: Tuple[float, float] = (1., 1.), allowed: Optional[torch.Tensor] = None):
        """(dist fp32 [Q, N], single): layer_weights[0] dist_top + layer_weights[1] dist_bottom of every query against
        every item; +inf where allowed[n] == 0."""
        if top_code is None and bottom_code is None:
            raise ValueError("search: give top_code, bottom_code or both")
        if any(float(w) < 0 for w in layer_weights):
            raise ValueError(f"layer_weights must be >= 0, got {tuple(layer_weights)}")
        checked = [(layer, weight) + self._checked(layer, code, mask)
                   for layer, code, mask, weight in (('top', top_code, mask_top, layer_weights[0]),
                                                     ('bottom', bottom_code, mask_bottom, layer_weights[1])) if code is not None]
        if len({c[2].shape[0] for c in checked}) != 1:
            raise ValueError("top_code and bottom_code hold different numbers of queries")
        jobs = [(layer,) + self._query(layer, code, mask, weight) + (single,) for layer, weight, code, mask, single in checked]
        Q, N = jobs[0][1].shape[0], len(self)
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(self.device))
        dist = torch.empty(Q, N, dtype=torch.float32, device=self.device)
        for n_done, (layer, query, weights, _) in enumerate(jobs):
            stored = self.top if layer == 'top' else self.bottom
            table = self.table(layer)
            cells, K = query.shape[1], table.shape[0]
            need = lib.isi_code_search_workspace_bytes(N, cells, K, Q)
            if self._workspace is None or self._workspace.numel() * 4 < need:
                self._workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.device)
            _hip.check(lib.isi_code_search_f32(
                stored.data_ptr(), query.data_ptr(), None if weights is None else weights.data_ptr(), table.data_ptr(),
                None if allowed is None else allowed.data_ptr(), dist.data_ptr(), N, cells, K, Q, int(n_done > 0),
                self._workspace.data_ptr(), self._workspace.numel() * 4, stream), "isi_code_search_f32")
        return dist, all(job[3] for job in jobs)

    def search(self, top_code=None, bottom_code=None, *, mask_top=None, mask_bottom=None,
               layer_weights: Tuple[float, float] = (1., 1.), k: int = 8,
               attribute_constraints: Optional[Mapping[str, object]] = None, exclude: Optional[Sequence[int]] = None):
        """The k nearest stored items: (indices int64 [k], distances float32 [k]), ordered by (distance, index) ascending;
        [Q, k] each for queries [Q, F, T] with Q > 1.  Codemaps are [F, T] or [1, F, T] in the stored shapes (ValueError
        otherwise); mask_* bool, True = "do not compare here" (the region about to be regenerated: weight 0), as is every
        query cell outside [0, n_embed) -- a query taken from an inpainting request carries the prior's mask token there.
        attribute_constraints: `sample_from_database`'s equality on decoded attributes; exclude: item indices left out.
        Fewer than k allowed items: as many as there are; none: LookupError.  CPU tensors: HipLibraryError."""
        if int(k) < 1:
            raise ValueError(f"k must be at least 1, not {k}")
        allowed = self.allowed(attribute_constraints, exclude)
        dist, single = self.distances(top_code, bottom_code, mask_top=mask_top, mask_bottom=mask_bottom,
                                      layer_weights=layer_weights, allowed=allowed)
        count = len(self) if allowed is None else int(allowed.sum())
        if count < 1:
            raise LookupError(f"no item of the index meets {dict(attribute_constraints or {})}"
                              + (f" outside {list(exclude)}" if exclude is not None and len(exclude) else ""))
        # a stable sort: equal distances keep the order of the item indices (torch.topk promises nothing for ties)
        values, order = torch.sort(dist, dim=1, stable=True)
        k = min(int(k), count)
        values, order = values[:, :k].contiguous(), order[:, :k].contiguous()
        return (order[0], values[0]) if single else (order, values)

    # ---- shift-invariant search (csrc/code_shift_search.hip)
    def _shift_plan(self, top_code, bottom_code, mask_top, mask_bottom, layer_weights, shift_range):
        """Validation and geometry of a shifted search, before any device work: (checked layers, lo, count) with the
        offsets lo .. lo + count - 1 in the columns of the first layer given."""
        if top_code is None and bottom_code is None:
            raise ValueError("search_shifted: give top_code, bottom_code or both")
        if any(float(w) < 0 for w in layer_weights):
            raise ValueError(f"layer_weights must be >= 0, got {tuple(layer_weights)}")
        checked = [(layer, weight) + self._checked(layer, code, mask, window=True)
                   for layer, code, mask, weight in (('top', top_code, mask_top, layer_weights[0]),
                                                     ('bottom', bottom_code, mask_bottom, layer_weights[1])) if code is not None]
        if len({c[2].shape[0] for c in checked}) != 1:
            raise ValueError("top_code and bottom_code hold different numbers of queries")
        stored = self.top if checked[0][0] == 'top' else self.bottom
        T, W = int(stored.shape[2]), int(checked[0][2].shape[2])
        if len(checked) == 2:
            ratio = self.bottom.shape[2] // self.top.shape[2]
            if ratio < 1 or ratio * self.top.shape[2] != self.bottom.shape[2]:
                raise ValueError(f"the bottom maps' {self.bottom.shape[2]} columns are no multiple of the top maps' "
                                 f"{self.top.shape[2]}: a two-layer shifted search has no common offset")
            if checked[1][2].shape[2] != ratio * W:
                raise ValueError(f"bottom_code: {checked[1][2].shape[2]} columns, but the top window's {W} columns span "
                                 f"{ratio * W} of the bottom layer")
        lo, hi = 0, T - W + 1
        if shift_range is not None:
            if len(shift_range) != 2:
                raise ValueError(f"shift_range: expected (lo, hi), got {shift_range}")
            lo, hi = max(lo, int(shift_range[0])), min(hi, int(shift_range[1]))
            if lo >= hi:
                raise ValueError(f"shift_range {tuple(shift_range)} holds no offset at which a window of {W} columns fits "
                                 f"the stored {T}")
        return checked, lo, hi - lo

    def _shifted_jobs(self, checked):
        jobs = []
        for layer, weight, code, mask, single in checked:
            query, weights = self._query(layer, code, mask, weight)
            jobs.append((layer, query, weights, int(code.shape[2]), single))
        return jobs

    def _shifted_group_size(self, jobs, count) -> int:
        """Queries per launch so that workspace + dist [g, S, N] stay under SHIFT_BUDGET_BYTES (at least 1)."""
        N = len(self)
        runs = max(-(-(self.top if layer == 'top' else self.bottom).shape[1] * W // 256) for layer, _, _, W, _ in jobs)
        per_query = (1 + (runs if runs > 1 else 0)) * count * N * 4
        return max(1, min(MAX_QUERIES, SHIFT_BUDGET_BYTES // per_query))

    def _shifted_into(self, jobs, q0: int, q1: int, first: int, count: int, dist: torch.Tensor) -> None:
        """dist [q1 - q0, count, N] (contiguous) of the queries q0 .. q1 - 1 at the offsets first .. first + count - 1."""
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(self.device))
        N, Q = len(self), q1 - q0
        ratio = 1 if len(jobs) == 1 else self.bottom.shape[2] // self.top.shape[2]
        for n_done, (layer, query, weights, W, _) in enumerate(jobs):
            stored = self.top if layer == 'top' else self.bottom
            table = self.table(layer)
            F, T, K = int(stored.shape[1]), int(stored.shape[2]), table.shape[0]
            step = ratio if n_done > 0 else 1
            need = lib.isi_code_shift_search_workspace_bytes(N, F, T, W, count, K, Q)
            if self._workspace is None or self._workspace.numel() * 4 < need:
                self._workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.device)
            _hip.check(lib.isi_code_shift_search_f32(
                stored.data_ptr(), query[q0:q1].data_ptr(), None if weights is None else weights[q0:q1].data_ptr(),
                table.data_ptr(), dist.data_ptr(), N, F, T, W, step * first, step, count, K, Q, int(n_done > 0),
                self._workspace.data_ptr(), self._workspace.numel() * 4, stream), "isi_code_shift_search_f32")

    def _shifted_groups(self, jobs, lo: int, count: int):
        """Yields (q0, q1, dist [q1 - q0, count, N]) group by group.  The launch starts at a multiple of 8 columns (the
        kernel reads aligned vectors from there); the offsets below `lo` are computed and dropped."""
        Q, N = jobs[0][1].shape[0], len(self)
        first = lo - lo % 8
        group = self._shifted_group_size(jobs, count + lo - first)
        for q0 in range(0, Q, group):
            q1 = min(Q, q0 + group)
            dist = torch.empty(q1 - q0, count + lo - first, N, dtype=torch.float32, device=self.device)
            self._shifted_into(jobs, q0, q1, first, count + lo - first, dist)
            yield q0, q1, (dist if first == lo else dist[:, lo - first:].contiguous())

    def distances_shifted(self, top_code=None, bottom_code=None, *, mask_top=None, mask_bottom=None,
                          layer_weights: Tuple[float, float] = (1., 1.), shift_range: Optional[Tuple[int, int]] = None):
        """dist fp32 [Q, S, N]: the distance of every query window to every item at every offset of `search_shifted`
        (dist[:, s] belongs to the offset lo + s, lo = the first allowed one).  Q S N floats: for callers that want
        every offset, not for the whole of a large database at once."""
        checked, lo, count = self._shift_plan(top_code, bottom_code, mask_top, mask_bottom, layer_weights, shift_range)
        jobs = self._shifted_jobs(checked)
        return torch.cat([dist for _, _, dist in self._shifted_groups(jobs, lo, count)], 0)

    def search_shifted(self, top_code=None, bottom_code=None, *, mask_top=None, mask_bottom=None,
                       layer_weights: Tuple[float, float] = (1., 1.), k: int = 8,
                       shift_range: Optional[Tuple[int, int]] = None,
                       attribute_constraints: Optional[Mapping[str, object]] = None, exclude: Optional[Sequence[int]] = None):
        """The k stored items that CONTAIN something nearest to a fragment, wherever it sits in time:
        (indices int64 [k], shifts int64 [k], distances float32 [k]); [Q, k] each for Q > 1 queries.
        top_code [F_t, W_t] (or [Q, F_t, W_t]) with W_t <= T_t, bottom_code [F_b, r W_t] with r = T_b / T_t; the window is
        laid over each item at every offset o with o + W <= T, an item counts once, at its best offset (the smallest of
        equal ones), and `shifts` holds that absolute offset -- in top columns whenever a top query is given, in bottom
        columns for a bottom query alone.  shift_range=(lo, hi): only offsets lo <= o < hi.  mask_*, layer_weights,
        attribute_constraints, exclude, the (distance, item index) order, LookupError / ValueError / HipLibraryError: as
        `search`.  The queries run in groups whose workspace and dist [Q, S, N] stay under SHIFT_BUDGET_BYTES; distances
        are query- and item-local, so the grouping changes no bit."""
        if int(k) < 1:
            raise ValueError(f"k must be at least 1, not {k}")
        checked, lo, count = self._shift_plan(top_code, bottom_code, mask_top, mask_bottom, layer_weights, shift_range)
        allowed = self.allowed(attribute_constraints, exclude)
        n_allowed = len(self) if allowed is None else int(allowed.sum())
        if n_allowed < 1:
            raise LookupError(f"no item of the index meets {dict(attribute_constraints or {})}"
                              + (f" outside {list(exclude)}" if exclude is not None and len(exclude) else ""))
        jobs = self._shifted_jobs(checked)
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(self.device))
        Q, N = jobs[0][1].shape[0], len(self)
        best = torch.empty(Q, N, dtype=torch.float32, device=self.device)
        best_shift = torch.empty(Q, N, dtype=torch.int32, device=self.device)
        for q0, q1, dist in self._shifted_groups(jobs, lo, count):
            _hip.check(lib.isi_code_shift_best_f32(dist.data_ptr(), None if allowed is None else allowed.data_ptr(),
                                                   best[q0:q1].data_ptr(), best_shift[q0:q1].data_ptr(), N, count, q1 - q0,
                                                   stream), "isi_code_shift_best_f32")
        values, order = torch.sort(best, dim=1, stable=True)
        k = min(int(k), n_allowed)
        values, order = values[:, :k].contiguous(), order[:, :k].contiguous()
        shifts = torch.gather(best_shift, 1, order).to(torch.int64) + lo
        single = all(job[4] for job in jobs)
        return (order[0], shifts[0], values[0]) if single else (order, shifts, values)
