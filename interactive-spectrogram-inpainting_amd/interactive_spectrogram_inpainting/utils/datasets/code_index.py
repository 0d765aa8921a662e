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
(csrc/code_shift_search.hip, specification tests/code_shift_search_spec.py).

That metric compares CODES with codes -- the product quantiser's symmetric distance, right for a query that is a codemap.
A query that is not -- an upload's encoder output before it is snapped to codes, a morph's per-cell blend of codes -- is
compared by the asymmetric distance instead (`search_soft`, `search_shifted_soft`; DESIGN.md section 6c.2, specification
tests/code_soft_search_spec.py): per cell a ROW of K floats takes the place of the table row,

    R[c][k]    = sum_d (z[c][d] - E[k][d])^2             built on the device from the vectors z (isi_code_query_rows_f32)
    dist(z, x) = sum_c w[c] R[c][x[c]]                   = sum_c w[c] |z[c] - E[x[c]]|^2; a cell of weight 0 counts nothing

through the same kernels with another stage, so a vector that is a codebook row gives the hard search's bits; any other
per-cell cost can be handed over as ready rows.  No CPU path: the index, the VQ-VAE and the queries must live on the
GPU.

All of the above compare column i of the query with column o + i of the item.  `search_warped` lets a sound unfold a
little faster or slower (csrc/code_warp_search.hip; DESIGN.md section 6c.3, specification tests/code_warp_search_spec.py):
query column i is matched to item column p(i), p(i+1) - p(i) in {0, 1, 2}, the drift p(i) - i inside a band, and the
distance is the least sum of `search_soft`'s column costs over all such paths; `warp_paths` returns the paths."""
from __future__ import annotations

import ctypes as C
import dataclasses
from collections import OrderedDict
from typing import Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ... import _hip

MAX_QUERIES = 64          # isi_code_search_f32: 1 <= Q <= 64 per launch
SHIFT_BUDGET_BYTES = 1 << 30      # search_shifted / distances_shifted: workspace + dist [Q, S, N] of one group of queries
MAX_DRIFTS = 64           # isi_code_warp_search_f32: hi - lo + 1 <= 64
MAX_PATH_ITEMS = 64       # isi_code_warp_path_f32: 1 <= M <= 64 per launch
ROWS_BUDGET_BYTES = 1 << 28       # search_soft / search_shifted_soft: rows [Q, C, K] built from vectors, one group of queries
                                  # (a flagship bottom map is 8 MB of rows per query: 32 queries at a time)


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


class _Stored(NamedTuple):
    """One layer of the index: the stored maps [N, F, T] and the layer's quantiser, K codes of D dimensions."""
    maps: torch.Tensor
    F: int
    T: int
    quantizer: object
    K: int
    D: int


@dataclasses.dataclass
class _QueryLayer:
    """One layer of a query, checked against the stored maps: data integer [Q, F, W] for kind 'code', floating
    [Q, F, W, D] for 'vectors', [Q, F, W, K] for 'rows'; mask bool [F, W] / [1 or Q, F, W] or None; W == T unless the
    search takes windows.  `_upload` adds what the kernels read."""
    layer: str
    kind: str
    data: torch.Tensor
    mask: Optional[torch.Tensor]
    weight: float
    single: bool
    W: int
    payload: Optional[torch.Tensor] = None            # uint16 [Q, C] codes, fp32 [Q, C, D] vectors or fp32 [Q, C, K] rows
    weights: Optional[torch.Tensor] = None            # fp32 [Q, C]; None: every cell weighs 1


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

    # ---- layers and tables
    def _layer(self, layer: str, given: Optional[str] = None) -> _Stored:
        """The 'top' or the 'bottom' layer of the index (ValueError, naming the argument `given`, when it holds none)."""
        maps, quantizer = (self.top, self.vqvae.quantize_t) if layer == 'top' else (self.bottom, self.vqvae.quantize_b)
        if maps is None:
            raise ValueError(f"{given or 'a ' + layer + ' layer'} given, but the index holds no {layer} maps")
        return _Stored(maps, int(maps.shape[1]), int(maps.shape[2]), quantizer, int(quantizer.n_embed), int(quantizer.dim))

    def _embed(self, layer: str) -> torch.Tensor:
        """The layer's codebook buffer [D, K], on the index's device (HipLibraryError otherwise)."""
        embed = self._layer(layer).quantizer.embed
        _hip.require_gpu(embed, f"quantize_{layer[0]}.embed")
        if embed.device != self.device:
            raise _hip.HipLibraryError(f"the VQ-VAE lives on {embed.device}, the index on {self.device}")
        return embed

    def table(self, layer: str) -> torch.Tensor:
        """The layer's code distance table [K, K] fp32, rebuilt when the codebook buffer changes."""
        embed = self._embed(layer)
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

    # ---- a query: validation on the host (wherever the tensors live), then the upload
    def _checked_layer(self, layer: str, code, vectors, rows, mask, weight: float, window: bool) -> _QueryLayer:
        """One layer of a query, given as exactly one of code / vectors / rows, checked against the stored maps
        (ValueError).  window: the query may be narrower than the stored maps, W columns with 1 <= W <= T."""
        given = [kind for kind, value in (('code', code), ('vectors', vectors), ('rows', rows)) if value is not None]
        if len(given) != 1:
            raise ValueError(f"the {layer} layer takes one of {layer}_code, {layer}_vectors and {layer}_rows, got "
                             + " and ".join(f"{layer}_{kind}" for kind in given))
        kind, name = given[0], f"{layer}_{given[0]}"
        stored = self._layer(layer, name)
        F, T = stored.F, stored.T
        data = torch.as_tensor({'code': code, 'vectors': vectors, 'rows': rows}[kind])
        tail = {'code': (), 'vectors': (stored.D,), 'rows': (stored.K,)}[kind]       # what follows [F, W] in a query's shape
        lead = data.dim() - 2 - len(tail)                                            # 1: a leading Q
        if lead not in (0, 1) or data.dtype.is_floating_point != (kind != 'code') or tuple(data.shape[lead + 2:]) != tail \
                or data.shape[lead] != F or not (1 <= data.shape[lead + 1] <= T if window else data.shape[lead + 1] == T):
            wanted = [str(F), f"W (1 <= W <= {T})" if window else str(T)] + [str(n) for n in tail]
            last = {'code': "", 'vectors': " and the layer's embedding dimension", 'rows': " and the layer's number of codes"}
            raise ValueError(f"{name}: expected {'integer' if kind == 'code' else 'floating-point'} [{', '.join(wanted)}] "
                             f"(or [Q, ...]) -- the stored maps' cells{last[kind]} -- got {data.dtype} {tuple(data.shape)}")
        single = lead == 0 or data.shape[0] == 1
        W = int(data.shape[lead + 1])
        data = data.reshape(-1, F, W, *tail)
        Q = data.shape[0]
        if not 1 <= Q <= MAX_QUERIES:
            raise ValueError(f"{name}: {Q} queries, a search takes 1..{MAX_QUERIES}")
        if mask is not None:
            mask = torch.as_tensor(mask)
            if mask.dtype != torch.bool or mask.dim() not in (2, 3) or tuple(mask.shape[-2:]) != (F, W) \
                    or (mask.dim() == 3 and mask.shape[0] not in (1, Q)):
                raise ValueError(f"mask_{layer}: expected bool [{F}, {W}] (or [Q, ...]), got {mask.dtype} {tuple(mask.shape)}")
        return _QueryLayer(layer, kind, data, mask, float(weight), single, W)

    def _checked_query(self, what: str, forms, masks, layer_weights, window: bool = False):
        """The layers given of a query for the method `what`, validated before any device work (ValueError): forms =
        ((top_code, top_vectors, top_rows), (bottom_code, ...)), masks = (mask_top, mask_bottom).  The layers hold equally
        many queries; two windows need a common offset: T_b = r T_t and a bottom window of r W columns."""
        if all(value is None for form in forms for value in form):
            raise ValueError(f"{what}: give a top layer, a bottom layer or both (as *_code, *_vectors or *_rows)")
        if any(float(w) < 0 for w in layer_weights):
            raise ValueError(f"layer_weights must be >= 0, got {tuple(layer_weights)}")
        layers = [self._checked_layer(layer, *form, mask, weight, window)
                  for layer, form, mask, weight in zip(('top', 'bottom'), forms, masks, layer_weights)
                  if any(value is not None for value in form)]
        if len({q.data.shape[0] for q in layers}) != 1:
            raise ValueError("the top and the bottom layer hold different numbers of queries")
        if window and len(layers) == 2:
            T_top, T_bottom = self.top.shape[2], self.bottom.shape[2]
            ratio = T_bottom // T_top
            if ratio < 1 or ratio * T_top != T_bottom:
                raise ValueError(f"the bottom maps' {T_bottom} columns are no multiple of the top maps' {T_top}: a two-layer "
                                 "search of windows has no common offset")
            if layers[1].W != ratio * layers[0].W:
                raise ValueError(f"bottom_{layers[1].kind}: the bottom window holds {layers[1].W} columns, but the top "
                                 f"window's {layers[0].W} columns span {ratio * layers[0].W} of the bottom layer")
        return layers

    def _plan(self, what: str, forms, masks, layer_weights, extent=None):
        """(checked layers, extent(T, W)) -- a search over windows hands in `extent`, which turns the stored T and the
        window's W, in the columns of the first layer given, into its offsets or its drifts; () for whole maps."""
        layers = self._checked_query(what, forms, masks, layer_weights, window=extent is not None)
        return layers, (() if extent is None else extent(self._layer(layers[0].layer).T, layers[0].W))

    def _upload(self, q: _QueryLayer) -> _QueryLayer:
        """The checked layer with payload and weights on the device (HipLibraryError for CPU tensors): a code layer's
        cells outside [0, K) become the mask token K."""
        stored = self._layer(q.layer)
        if not q.data.is_cuda or (q.mask is not None and not q.mask.is_cuda) or not stored.maps.is_cuda:
            raise _hip.HipLibraryError(f"{q.layer}_{q.kind} / mask_{q.layer} / the index live on "
                                       f"{q.data.device} / {None if q.mask is None else q.mask.device} / {stored.maps.device}: "
                                       "this package computes only on an MI355X (HIP kernels, no CPU fallback)")
        Q, shape = q.data.shape[0], (stored.F, q.W)
        if q.kind == 'code':
            code = q.data.to(self.device, torch.int64)
            payload = torch.where((code < 0) | (code > stored.K), stored.K, code).to(torch.uint16).reshape(Q, -1).contiguous()
        else:
            payload = q.data.to(self.device, torch.float32).reshape(Q, stored.F * q.W, -1).contiguous()
        weights = None
        if q.mask is not None or q.weight != 1.0:
            keep = torch.ones(Q, *shape, dtype=torch.bool, device=self.device) if q.mask is None \
                else ~q.mask.to(self.device).reshape(-1, *shape).expand(Q, *shape)
            weights = (keep.to(torch.float32) * q.weight).reshape(Q, -1).contiguous()
        return dataclasses.replace(q, payload=payload, weights=weights)

    def _rows_group_size(self, layers, counted=('vectors',)) -> int:
        """Queries per launch so that the rows made for them, [g, C, K] fp32 per layer of a kind in `counted`, stay under
        ROWS_BUDGET_BYTES (at least 1).  Rows the caller hands over exist already and are never counted."""
        per_query = max([q.payload.shape[1] * self._layer(q.layer).K * 4 for q in layers if q.kind in counted] or [0])
        return MAX_QUERIES if per_query == 0 else max(1, min(MAX_QUERIES, ROWS_BUDGET_BYTES // per_query))

    def _rows_of(self, q: _QueryLayer, q0: int, q1: int) -> torch.Tensor:
        """rows fp32 [q1 - q0, C, K] of a vectors or rows layer, built on the device for a vectors layer."""
        if q.kind == 'rows':
            return q.payload[q0:q1]
        self._embed(q.layer)
        return self._layer(q.layer).quantizer.distance_rows(q.payload[q0:q1])

    def _grow_workspace(self, need: int) -> None:
        if self._workspace is None or self._workspace.numel() * 4 < need:
            self._workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.device)

    # ---- what the searches share around the distances: the order of their steps, who is admitted, the ranking
    def _distances(self, what: str, forms, masks, layer_weights, distances, allowed, extent=None):
        """(dist fp32 [Q, N], single) of the aligned or the warped routine `distances`: plan, upload, launch."""
        layers, extent = self._plan(what, forms, masks, layer_weights, extent)
        return distances([self._upload(q) for q in layers], *extent, allowed), all(q.single for q in layers)

    def _search(self, what: str, forms, masks, layer_weights, k: int, attribute_constraints, exclude, distances, extent=None,
                rank=None):
        """Every search, in one order: k and the query are checked (ValueError), then who is admitted (LookupError), and
        only then anything is uploaded (HipLibraryError) and launched -- `distances(layers, *extent, allowed)` -- and
        ranked: by `rank`, or the k nearest of dist [Q, N]."""
        if int(k) < 1:
            raise ValueError(f"k must be at least 1, not {k}")
        layers, extent = self._plan(what, forms, masks, layer_weights, extent)
        allowed = self.allowed(attribute_constraints, exclude)
        n_allowed = self._admitted(allowed, attribute_constraints, exclude)
        found = distances([self._upload(q) for q in layers], *extent, allowed)
        single = all(q.single for q in layers)
        if rank is not None:
            return rank(found, layers[0].data.shape[0], *extent, allowed, n_allowed, k, single)
        values, order = self._nearest(found, k, n_allowed)
        return (order[0], values[0]) if single else (order, values)

    def _admitted(self, allowed: Optional[torch.Tensor], attribute_constraints, exclude) -> int:
        """How many items `allowed` admits (LookupError when none)."""
        count = len(self) if allowed is None else int(allowed.sum())
        if count < 1:
            raise LookupError(f"no item of the index meets {dict(attribute_constraints or {})}"
                              + (f" outside {list(exclude)}" if exclude is not None and len(exclude) else ""))
        return count

    @staticmethod
    def _nearest(dist: torch.Tensor, k: int, count: int):
        """(values, order) [Q, min(k, count)] of dist [Q, N], by (distance, item index) ascending.  A stable sort: equal
        distances keep the order of the item indices (torch.topk promises nothing for ties)."""
        values, order = torch.sort(dist, dim=1, stable=True)
        k = min(int(k), count)
        return values[:, :k].contiguous(), order[:, :k].contiguous()

    def _best_over_shifts(self, groups, Q: int, lo: int, count: int, allowed, n_allowed: int, k: int, single: bool):
        """The result of a shifted search from its groups (q0, q1, dist [q1 - q0, count, N]): every item at its best offset
        (isi_code_shift_best_f32), ranked, the offsets made absolute."""
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(self.device))
        N = len(self)
        best = torch.empty(Q, N, dtype=torch.float32, device=self.device)
        best_shift = torch.empty(Q, N, dtype=torch.int32, device=self.device)
        for q0, q1, dist in groups:
            _hip.check(lib.isi_code_shift_best_f32(dist.data_ptr(), None if allowed is None else allowed.data_ptr(),
                                                   best[q0:q1].data_ptr(), best_shift[q0:q1].data_ptr(), N, count, q1 - q0,
                                                   stream), "isi_code_shift_best_f32")
        values, order = self._nearest(best, k, n_allowed)
        shifts = torch.gather(best_shift, 1, order).to(torch.int64) + lo
        return (order[0], shifts[0], values[0]) if single else (order, shifts, values)

    # ---- aligned search (csrc/code_search.hip)
    def _aligned_distances(self, layers, allowed: Optional[torch.Tensor]) -> torch.Tensor:
        """dist fp32 [Q, N] of uploaded layers: a code layer through isi_code_search_f32, a vectors or rows layer through
        isi_code_search_rows_f32, the layers after the first accumulated; the queries in groups that keep the rows built
        from vectors under ROWS_BUDGET_BYTES."""
        Q, N = layers[0].payload.shape[0], len(self)
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(self.device))
        dist = torch.empty(Q, N, dtype=torch.float32, device=self.device)
        group = self._rows_group_size(layers)
        for q0 in range(0, Q, group):
            q1 = min(Q, q0 + group)
            for n_done, q in enumerate(layers):
                stored = self._layer(q.layer)
                cells = q.payload.shape[1]
                self._grow_workspace(lib.isi_code_search_workspace_bytes(N, cells, stored.K, q1 - q0))
                common = (None if allowed is None else allowed.data_ptr(), dist[q0:q1].data_ptr(), N, cells, stored.K, q1 - q0,
                          int(n_done > 0), self._workspace.data_ptr(), self._workspace.numel() * 4, stream)
                w_ptr = None if q.weights is None else q.weights[q0:q1].data_ptr()
                if q.kind == 'code':
                    _hip.check(lib.isi_code_search_f32(stored.maps.data_ptr(), q.payload[q0:q1].data_ptr(), w_ptr,
                                                       self.table(q.layer).data_ptr(), *common), "isi_code_search_f32")
                else:
                    rows = self._rows_of(q, q0, q1)
                    _hip.check(lib.isi_code_search_rows_f32(stored.maps.data_ptr(), rows.data_ptr(), w_ptr, *common),
                               "isi_code_search_rows_f32")
        return dist

    def distances(self, top_code=None, bottom_code=None, *, mask_top=None, mask_bottom=None,
                  layer_weights: Tuple[float, float] = (1., 1.), allowed: Optional[torch.Tensor] = None):
        """(dist fp32 [Q, N], single): layer_weights[0] dist_top + layer_weights[1] dist_bottom of every query against
        every item; +inf where allowed[n] == 0."""
        return self._distances("search", ((top_code, None, None), (bottom_code, None, None)), (mask_top, mask_bottom),
                               layer_weights, self._aligned_distances, allowed)

    def search(self, top_code=None, bottom_code=None, *, mask_top=None, mask_bottom=None,
               layer_weights: Tuple[float, float] = (1., 1.), k: int = 8,
               attribute_constraints: Optional[Mapping[str, object]] = None, exclude: Optional[Sequence[int]] = None):
        """The k nearest stored items: (indices int64 [k], distances float32 [k]), ordered by (distance, index) ascending;
        [Q, k] each for queries [Q, F, T] with Q > 1.  Codemaps are [F, T] or [1, F, T] in the stored shapes (ValueError
        otherwise); mask_* bool, True = "do not compare here" (the region about to be regenerated: weight 0), as is every
        query cell outside [0, n_embed) -- a query taken from an inpainting request carries the prior's mask token there.
        attribute_constraints: `sample_from_database`'s equality on decoded attributes; exclude: item indices left out.
        Fewer than k allowed items: as many as there are; none: LookupError.  CPU tensors: HipLibraryError."""
        return self._search("search", ((top_code, None, None), (bottom_code, None, None)), (mask_top, mask_bottom),
                            layer_weights, k, attribute_constraints, exclude, self._aligned_distances)

    # ---- shift-invariant search (csrc/code_shift_search.hip)
    @staticmethod
    def _shift_offsets(T: int, W: int, shift_range):
        """(lo, count): the offsets lo .. lo + count - 1 at which a window of W columns fits the stored T, inside
        shift_range (ValueError when there is none)."""
        lo, hi = 0, T - W + 1
        if shift_range is not None:
            if len(shift_range) != 2:
                raise ValueError(f"shift_range: expected (lo, hi), got {shift_range}")
            lo, hi = max(lo, int(shift_range[0])), min(hi, int(shift_range[1]))
            if lo >= hi:
                raise ValueError(f"shift_range {tuple(shift_range)} holds no offset at which a window of {W} columns fits "
                                 f"the stored {T}")
        return lo, hi - lo

    def _shifted_group_size(self, layers, count) -> int:
        """Queries per launch so that workspace + dist [g, S, N] stay under SHIFT_BUDGET_BYTES (at least 1)."""
        N = len(self)
        runs = max(-(-self._layer(q.layer).F * q.W // 256) for q in layers)
        per_query = (1 + (runs if runs > 1 else 0)) * count * N * 4
        return max(1, min(MAX_QUERIES, SHIFT_BUDGET_BYTES // per_query))

    def _shifted_groups(self, layers, lo: int, count: int, allowed=None):
        """Yields (q0, q1, dist [q1 - q0, count, N]) group by group, for the hard and the soft shifted searches: a code layer
        through isi_code_shift_search_f32, a vectors or rows layer through isi_code_shift_search_rows_f32.  The launch
        starts at a multiple of 8 columns (the kernel reads aligned vectors from there); the offsets below `lo` are computed
        and dropped.  (`allowed` plays no part at a single offset: `_best_over_shifts` applies it.)"""
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(self.device))
        Q, N = layers[0].payload.shape[0], len(self)
        first = lo - lo % 8
        S = count + lo - first
        group = min(self._shifted_group_size(layers, S), self._rows_group_size(layers))
        ratio = 1 if len(layers) == 1 else self.bottom.shape[2] // self.top.shape[2]
        for q0 in range(0, Q, group):
            q1 = min(Q, q0 + group)
            dist = torch.empty(q1 - q0, S, N, dtype=torch.float32, device=self.device)
            for n_done, q in enumerate(layers):
                stored = self._layer(q.layer)
                step = ratio if n_done > 0 else 1
                self._grow_workspace(lib.isi_code_shift_search_workspace_bytes(N, stored.F, stored.T, q.W, S, stored.K, q1 - q0))
                common = (dist.data_ptr(), N, stored.F, stored.T, q.W, step * first, step, S, stored.K, q1 - q0, int(n_done > 0),
                          self._workspace.data_ptr(), self._workspace.numel() * 4, stream)
                w_ptr = None if q.weights is None else q.weights[q0:q1].data_ptr()
                if q.kind == 'code':
                    _hip.check(lib.isi_code_shift_search_f32(stored.maps.data_ptr(), q.payload[q0:q1].data_ptr(), w_ptr,
                                                             self.table(q.layer).data_ptr(), *common), "isi_code_shift_search_f32")
                else:
                    rows = self._rows_of(q, q0, q1)
                    _hip.check(lib.isi_code_shift_search_rows_f32(stored.maps.data_ptr(), rows.data_ptr(), w_ptr, *common),
                               "isi_code_shift_search_rows_f32")
            yield q0, q1, (dist if first == lo else dist[:, lo - first:].contiguous())

    def _distances_shifted(self, what: str, forms, masks, layer_weights, shift_range) -> torch.Tensor:
        """dist fp32 [Q, S, N] of every offset: plan, upload, launch, the groups joined."""
        layers, (lo, count) = self._plan(what, forms, masks, layer_weights, lambda T, W: self._shift_offsets(T, W, shift_range))
        return torch.cat([dist for _, _, dist in self._shifted_groups([self._upload(q) for q in layers], lo, count)], 0)

    def distances_shifted(self, top_code=None, bottom_code=None, *, mask_top=None, mask_bottom=None,
                          layer_weights: Tuple[float, float] = (1., 1.), shift_range: Optional[Tuple[int, int]] = None):
        """dist fp32 [Q, S, N]: the distance of every query window to every item at every offset of `search_shifted`
        (dist[:, s] belongs to the offset lo + s, lo = the first allowed one).  Q S N floats: for callers that want
        every offset, not for the whole of a large database at once."""
        return self._distances_shifted("search_shifted", ((top_code, None, None), (bottom_code, None, None)),
                                       (mask_top, mask_bottom), layer_weights, shift_range)

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
        return self._search("search_shifted", ((top_code, None, None), (bottom_code, None, None)), (mask_top, mask_bottom),
                            layer_weights, k, attribute_constraints, exclude, self._shifted_groups,
                            lambda T, W: self._shift_offsets(T, W, shift_range), self._best_over_shifts)

    # ---- search by encoder vectors: per-cell distance rows
    def distances_soft(self, top_code=None, bottom_code=None, *, top_vectors=None, bottom_vectors=None, top_rows=None,
                       bottom_rows=None, mask_top=None, mask_bottom=None, layer_weights: Tuple[float, float] = (1., 1.),
                       allowed: Optional[torch.Tensor] = None):
        """(dist fp32 [Q, N], single) as `distances`, each layer given as exactly one of codes (`distances`' launch), vectors
        [Q, F, T, D] (or [F, T, D]) -- dist = sum_c w[c] |z[c] - E[x[c]]|^2, the rows built on the device -- or ready rows
        [Q, F, T, K] of any per-cell cost."""
        return self._distances("search_soft", ((top_code, top_vectors, top_rows), (bottom_code, bottom_vectors, bottom_rows)),
                               (mask_top, mask_bottom), layer_weights, self._aligned_distances, allowed)

    def search_soft(self, top_code=None, bottom_code=None, *, top_vectors=None, bottom_vectors=None, top_rows=None,
                    bottom_rows=None, mask_top=None, mask_bottom=None, layer_weights: Tuple[float, float] = (1., 1.), k: int = 8,
                    attribute_constraints: Optional[Mapping[str, object]] = None, exclude: Optional[Sequence[int]] = None):
        """`search` for queries that are no codemaps: the k stored items nearest to per-cell VECTORS -- an encoder's output
        before it is snapped to codes (`VQVAE.encode_vectors`), or a blend of codes (`embed_mix`) -- by
        dist(z, x) = sum_c w[c] |z[c] - E[x[c]]|^2.  Per layer give exactly one of `*_code` (compared through the code
        distance table, as `search` does), `*_vectors` [F, T, D] (or [Q, F, T, D]; D the layer's embedding dimension) or
        `*_rows` [Q, F, T, K], ready per-cell costs of every code; the layers add up as in `search`, so an upload's top
        vectors can be searched beside hard bottom codes.  There is no mask token in a vector: mask_* (True = weight 0) is
        the only mask, and a masked cell counts nothing whatever its vector holds.  Vectors that are codebook rows bit for
        bit give `search`'s distances bit for bit.  Everything else -- layer_weights, k, attribute_constraints, exclude,
        the (distance, index) order, LookupError / ValueError / HipLibraryError -- is `search`'s.  Rows are built for at
        most ROWS_BUDGET_BYTES of queries at a time; distances are query-local, so the grouping changes no bit."""
        return self._search("search_soft", ((top_code, top_vectors, top_rows), (bottom_code, bottom_vectors, bottom_rows)),
                            (mask_top, mask_bottom), layer_weights, k, attribute_constraints, exclude, self._aligned_distances)

    def distances_shifted_soft(self, top_code=None, bottom_code=None, *, top_vectors=None, bottom_vectors=None, top_rows=None,
                               bottom_rows=None, mask_top=None, mask_bottom=None,
                               layer_weights: Tuple[float, float] = (1., 1.), shift_range: Optional[Tuple[int, int]] = None):
        """dist fp32 [Q, S, N] as `distances_shifted`, for windows given per layer as codes, vectors [Q, F, W, D] or rows
        [Q, F, W, K] (`search_shifted_soft`)."""
        return self._distances_shifted("search_shifted_soft", ((top_code, top_vectors, top_rows),
                                                               (bottom_code, bottom_vectors, bottom_rows)),
                                       (mask_top, mask_bottom), layer_weights, shift_range)

    def search_shifted_soft(self, top_code=None, bottom_code=None, *, top_vectors=None, bottom_vectors=None, top_rows=None,
                            bottom_rows=None, mask_top=None, mask_bottom=None, layer_weights: Tuple[float, float] = (1., 1.),
                            k: int = 8, shift_range: Optional[Tuple[int, int]] = None,
                            attribute_constraints: Optional[Mapping[str, object]] = None,
                            exclude: Optional[Sequence[int]] = None):
        """`search_shifted` for windows that are no codemaps: per layer exactly one of `*_code` [F, W], `*_vectors`
        [F, W, D] or `*_rows` [Q, F, W, K] (a leading Q as in `search_soft`), the bottom window r = T_b / T_t times as
        wide as the top one.  Returns (indices, shifts, distances) as `search_shifted` does, with its offsets, shift_range,
        masks, constraints, ordering and errors; the zero-weight rule and the bitwise agreement with the hard search on
        vectors that are codebook rows are `search_soft`'s.  The groups of queries respect both SHIFT_BUDGET_BYTES and
        ROWS_BUDGET_BYTES."""
        return self._search("search_shifted_soft", ((top_code, top_vectors, top_rows), (bottom_code, bottom_vectors, bottom_rows)),
                            (mask_top, mask_bottom), layer_weights, k, attribute_constraints, exclude, self._shifted_groups,
                            lambda T, W: self._shift_offsets(T, W, shift_range), self._best_over_shifts)

    # ---- time-warped search (csrc/code_warp_search.hip)
    @staticmethod
    def _drift_band(T: int, W: int, drift):
        """(lo, hi): the drifts of a warped search of W query columns over the stored T (ValueError)."""
        try:
            lo, hi = (int(d) for d in drift)
        except (TypeError, ValueError):
            raise ValueError(f"drift: expected (lo, hi), got {drift}") from None
        if lo > hi:
            raise ValueError(f"drift {(lo, hi)}: lo must not exceed hi")
        if hi - lo + 1 > MAX_DRIFTS:
            raise ValueError(f"drift {(lo, hi)} holds {hi - lo + 1} drifts, a warped search takes at most {MAX_DRIFTS}")
        if hi < 0 or lo > T - 1 or W - 1 + hi < 0 or W - 1 + lo > T - 1:
            raise ValueError(f"drift {(lo, hi)} leaves the first or the last of {W} query columns without a column of the "
                             f"stored {T}")
        return lo, hi

    def _warp_rows(self, q: _QueryLayer, q0: int, q1: int):
        """(rows fp32 [g, C, K], weights fp32 [g, C] or None) of one layer of a warped query: a code layer as rows gathered
        from the code distance table, its mask-token cells under weight 0."""
        w = None if q.weights is None else q.weights[q0:q1]
        if q.kind != 'code':
            return self._rows_of(q, q0, q1), w
        table = self.table(q.layer)
        K = table.shape[0]
        query = q.payload[q0:q1].view(torch.int16).to(torch.int64).bitwise_and(0xFFFF)
        token = query >= K
        rows = table[torch.where(token, 0, query)].contiguous()
        if w is None:
            w = torch.ones(query.shape, dtype=torch.float32, device=self.device)
        return rows, torch.where(token, 0.0, w).contiguous()

    def _warp_parts(self, layers, q0: int, q1: int):
        """(isi_warp_part array, T, the tensors it points into) of the queries q0 .. q1 - 1."""
        ratio = 1 if len(layers) == 1 else self.bottom.shape[2] // self.top.shape[2]
        parts = (_hip.isi_warp_part * len(layers))()
        keep = []
        for p, q in enumerate(layers):
            stored = self._layer(q.layer)
            rows, w = self._warp_rows(q, q0, q1)
            keep += [rows, w]
            parts[p].codes, parts[p].rows = stored.maps.data_ptr(), rows.data_ptr()
            parts[p].weights = None if w is None else w.data_ptr()
            parts[p].F, parts[p].r, parts[p].K = stored.F, (ratio if p > 0 else 1), int(rows.shape[2])
        return parts, self._layer(layers[0].layer).T, keep

    def _warped_distances(self, layers, lo: int, hi: int, allowed: Optional[torch.Tensor]) -> torch.Tensor:
        """dist fp32 [Q, N] of uploaded layers (isi_code_warp_search_f32), the queries in groups that keep the rows built
        or gathered for them under ROWS_BUDGET_BYTES."""
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(self.device))
        Q, N = layers[0].payload.shape[0], len(self)
        dist = torch.empty(Q, N, dtype=torch.float32, device=self.device)
        group = self._rows_group_size(layers, ('code', 'vectors'))
        for q0 in range(0, Q, group):
            q1 = min(Q, q0 + group)
            parts, T, keep = self._warp_parts(layers, q0, q1)
            _hip.check(lib.isi_code_warp_search_f32(parts, len(layers), None if allowed is None else allowed.data_ptr(),
                                                    dist[q0:q1].data_ptr(), None, N, T, layers[0].W, lo, hi, q1 - q0, stream),
                       "isi_code_warp_search_f32")
            del keep
        return dist

    def distances_warped(self, top_code=None, bottom_code=None, *, top_vectors=None, bottom_vectors=None, top_rows=None,
                         bottom_rows=None, mask_top=None, mask_bottom=None, layer_weights: Tuple[float, float] = (1., 1.),
                         drift: Tuple[int, int] = (-4, 4), allowed: Optional[torch.Tensor] = None):
        """(dist fp32 [Q, N], single): the warped distance of `search_warped` of every query to every item; +inf where
        allowed[n] == 0."""
        return self._distances("search_warped", ((top_code, top_vectors, top_rows), (bottom_code, bottom_vectors, bottom_rows)),
                               (mask_top, mask_bottom), layer_weights, self._warped_distances, allowed,
                               lambda T, W: self._drift_band(T, W, drift))

    def search_warped(self, top_code=None, bottom_code=None, *, top_vectors=None, bottom_vectors=None, top_rows=None,
                      bottom_rows=None, mask_top=None, mask_bottom=None, layer_weights: Tuple[float, float] = (1., 1.),
                      k: int = 8, drift: Tuple[int, int] = (-4, 4),
                      attribute_constraints: Optional[Mapping[str, object]] = None, exclude: Optional[Sequence[int]] = None):
        """The k stored items nearest to a sound that may unfold a little faster or slower than the query:
        (indices int64 [k], distances float32 [k]); [Q, k] each for Q > 1 queries.  Query column i is matched to one item
        column p(i) with p(i+1) - p(i) in {0, 1, 2} and lo <= p(i) - i <= hi for drift=(lo, hi); every query column counts
        once, and the distance is the least sum of column costs over all such paths (specification
        tests/code_warp_search_spec.py).  A column's cost is `search_soft`'s sum over its cells.  Per layer give exactly one
        of `*_code`, `*_vectors` or `*_rows`, as a whole map or as a window [F, W] of 1 <= W <= T columns (the bottom
        window r = T_b / T_t times as wide as the top one); drift is measured in top columns whenever a top layer is
        given, and hi - lo + 1 <= 64.  drift=(o, o) is the shifted search's alignment at offset o.  Masks, layer_weights,
        the (distance, index) order, attribute_constraints, exclude, LookupError / ValueError / HipLibraryError and the
        grouping of the queries under ROWS_BUDGET_BYTES are `search_soft`'s."""
        return self._search("search_warped", ((top_code, top_vectors, top_rows), (bottom_code, bottom_vectors, bottom_rows)),
                            (mask_top, mask_bottom), layer_weights, k, attribute_constraints, exclude, self._warped_distances,
                            lambda T, W: self._drift_band(T, W, drift))

    def warp_paths(self, indices, top_code=None, bottom_code=None, *, top_vectors=None, bottom_vectors=None, top_rows=None,
                   bottom_rows=None, mask_top=None, mask_bottom=None, layer_weights: Tuple[float, float] = (1., 1.),
                   drift: Tuple[int, int] = (-4, 4)):
        """The alignments behind `search_warped`'s distances: for items `indices` [k] (or [Q, k]) and the same query, the
        item column p(i) matched to every query column, int64 [k, W] (or [Q, k, W]).  Among paths of equal cost the one
        that prefers step over hold over skip, backtracked from the smallest end column."""
        forms = (top_code, top_vectors, top_rows), (bottom_code, bottom_vectors, bottom_rows)
        layers, (lo, hi) = self._plan("warp_paths", forms, (mask_top, mask_bottom), layer_weights,
                                      lambda T, W: self._drift_band(T, W, drift))
        layers = [self._upload(q) for q in layers]
        Q, N, W, single = layers[0].payload.shape[0], len(self), layers[0].W, all(q.single for q in layers)
        items = torch.as_tensor(indices)
        if items.dtype.is_floating_point or items.dtype == torch.bool or items.dim() not in (1, 2) or items.numel() == 0 \
                or (items.dim() == 2 and items.shape[0] != Q) or (items.dim() == 1 and Q != 1):
            raise ValueError(f"indices: expected item indices [k] (or [{Q}, k] for {Q} queries), got "
                             f"{items.dtype} {tuple(items.shape)}")
        items = items.reshape(Q, -1).to(self.device, torch.int64)
        if int(items.min()) < -N or int(items.max()) >= N:
            raise IndexError(f"indices outside an index of {N} items")
        items = items % N
        lib, stream = _hip.lib(), C.c_void_p(_hip.stream_ptr(self.device))
        path = torch.empty(Q, items.shape[1], W, dtype=torch.int32, device=self.device)
        group = self._rows_group_size(layers, ('code', 'vectors'))
        for q0 in range(0, Q, group):
            q1 = min(Q, q0 + group)
            parts, T, keep = self._warp_parts(layers, q0, q1)
            for m0 in range(0, items.shape[1], MAX_PATH_ITEMS):
                chosen = items[q0:q1, m0:m0 + MAX_PATH_ITEMS].contiguous()
                M = chosen.shape[1]
                out = torch.empty(q1 - q0, M, W, dtype=torch.int32, device=self.device)
                dist = torch.empty(q1 - q0, M, dtype=torch.float32, device=self.device)
                self._grow_workspace(lib.isi_code_warp_path_workspace_bytes(M, W, lo, hi, q1 - q0))
                _hip.check(lib.isi_code_warp_path_f32(parts, len(layers), chosen.data_ptr(), M, out.data_ptr(), dist.data_ptr(),
                                                      self._workspace.data_ptr(), self._workspace.numel() * 4, N, T, W, lo, hi,
                                                      q1 - q0, stream), "isi_code_warp_path_f32")
                path[q0:q1, m0:m0 + M] = out
            del keep
        path = path.to(torch.int64)
        return path[0] if single and torch.as_tensor(indices).dim() == 1 else path
