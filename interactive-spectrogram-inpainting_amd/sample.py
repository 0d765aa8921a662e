"""Autoregressive / inpainting sampling of codemaps on MI355X.

Drop-in for `sample_model` and `top_k_top_p_filtering` of the reference's
`sample.py:36-65,131-347` (the CLI, audio and PNG writing of that script are
harness code outside the compute path).  Contract kept:
positions with `mask == False` keep `initial_code`; masked positions are sampled
left to right in the target helper's order; `temperature` divides the logits;
the result is an int64 codemap `[B, F, T]`.

Differences by design: the decoder runs incrementally on cached keys / values
(same logits as the reference's full pass per token, O(S) instead of O(S^2) layer
passes); filtering + softmax + the categorical draw are one kernel on the single
row that is consumed; the draw uses uniforms from `generator` (or given `uniforms`)
instead of torch.multinomial's stream.
"""
from __future__ import annotations

import os
from typing import Iterable, Mapping, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from interactive_spectrogram_inpainting.priors import _ops
from interactive_spectrogram_inpainting.priors._decode import NativeSampler, kv_cache_format
from interactive_spectrogram_inpainting.priors.transformer import Seq2SeqInputKind, VQNSynthTransformer


def top_k_top_p_filtering(logits: torch.Tensor, top_k: int = 0, top_p: float = 0.0,
                          filter_value: float = -float('Inf')) -> torch.Tensor:
    """Filter logits `[..., n_class]` in place (like the reference) with top-k and/or
    nucleus filtering; runs `isi_sample_row_f32`'s filtering stage on every row."""
    if filter_value != -float('Inf'):
        raise NotImplementedError("only filter_value = -inf is built")
    rows = logits.reshape(-1, logits.shape[-1])
    u = torch.zeros(rows.shape[0], device=logits.device)
    _, filt = _ops.sample_rows(rows, 1.0, top_k, top_p, u, return_filtered=True)
    logits.copy_(filt.reshape(logits.shape))
    return logits


def _kv_cache_dtype(kv_cache_dtype: Optional[torch.dtype]) -> torch.dtype:
    """The key/value cache format of the KV-cached loop: the argument, or (None) the switch ISI_DECODE_KV = f32 | bf16
    (default f32).  bf16 halves the bytes a position streams from the two caches; keys and values then carry 8
    significand bits and the sampled codes may differ from an fp32-cache run's."""
    if kv_cache_dtype is None:
        name = os.environ.get("ISI_DECODE_KV", "f32")
        if name not in ("f32", "bf16"):
            raise ValueError(f"ISI_DECODE_KV must be f32 or bf16, not {name!r}")
        kv_cache_dtype = torch.bfloat16 if name == "bf16" else torch.float32
    kv_cache_format(kv_cache_dtype)            # ValueError for anything but float32 / bfloat16
    return kv_cache_dtype


def _per_row(value, batch_size: int, name: str):
    """A sampling parameter given once or per row: (scalar, None) when every row shares it, else (first, tensor [B])."""
    if not torch.is_tensor(value) and not isinstance(value, (list, tuple, np.ndarray)):
        return value, None
    t = torch.as_tensor(value).reshape(-1).cpu()
    if t.numel() != batch_size:
        raise ValueError(f"{name}: {t.numel()} values for a batch of {batch_size}")
    if bool((t == t[0]).all()):
        return t[0].item(), None
    return t[0].item(), t


def _ragged_plan(mask_rows: np.ndarray, i_off: int):
    """Steps of a ragged batch: row b walks from the decoder position of its first masked token to that of its last, one
    position per step, then idles at its last position; it commits where its own token is masked.  A row with nothing
    masked idles at position 0 and never commits.  Returns (pos, commit) [n_steps, B] and the prefill length."""
    B = mask_rows.shape[0]
    spans = []
    for b in range(B):
        idx = np.flatnonzero(mask_rows[b])
        spans.append((idx[0] + i_off, idx[-1] + i_off + 1) if idx.size else None)
    n_steps = max((e - f for f, e in (sp for sp in spans if sp)), default=0)
    prefill = max((f for f, _ in (sp for sp in spans if sp)), default=0)
    t = np.arange(n_steps)[:, None]
    pos = np.zeros((n_steps, B), dtype=np.int32)
    commit = np.zeros((n_steps, B), dtype=np.uint8)
    for b, sp in enumerate(spans):
        if sp is None:
            continue
        f, e = sp
        p = np.minimum(f + t[:, 0], e - 1)
        pos[:, b] = p
        commit[:, b] = (t[:, 0] < e - f) & mask_rows[b][p - i_off]
    return pos, commit, prefill


def codes_in_use(codemaps, n_class: int) -> torch.Tensor:
    """bool [n_class]: the classes that occur in a codemap or in any of several (a tensor of any shape, or a collection of
    tensors) -- the codes an encoder has produced, or the palette of a sound; `sample_model(allowed_codes=...)` takes it as
    it is.  Values outside [0, n_class) (the top prior's mask token) are not classes and are left out."""
    maps = [codemaps] if torch.is_tensor(codemaps) else list(codemaps)
    used = torch.zeros(int(n_class), dtype=torch.bool)
    for m in maps:
        v = torch.as_tensor(m).reshape(-1).long().cpu()
        used[v[(v >= 0) & (v < n_class)]] = True
    return used


def _code_bias_rows(model, batch_size: int, code_bias, code_bias_map, allowed_codes):
    """The options `code_bias` / `code_bias_map` / `allowed_codes` of `sample_model`, checked: a float32 table [R, n_class]
    and an int64 map [1 or B, F, T] of its rows in codemap layout (None: row 0 in every cell), host tensors, or
    (None, None) with the options off.  Every refusal is a ValueError raised here, before any device work."""
    if code_bias is None and allowed_codes is None:
        if code_bias_map is not None:
            raise ValueError("code_bias_map selects rows of code_bias (or the one row of allowed_codes): neither is given")
        return None, None
    if code_bias is not None and allowed_codes is not None:
        raise ValueError("allowed_codes is shorthand for a code_bias row of 0 and -inf: give one of the two")
    n = int(model.n_class_target)
    if allowed_codes is not None:
        a = allowed_codes if torch.is_tensor(allowed_codes) else torch.as_tensor(
            np.asarray(allowed_codes if isinstance(allowed_codes, (list, tuple, np.ndarray)) else sorted(allowed_codes)))
        a = a.detach().cpu()
        if a.dtype == torch.bool:
            if tuple(a.shape) != (n,):
                raise ValueError(f"allowed_codes: a bool mask is [{n}] (n_class_target), not {tuple(a.shape)}")
            allowed = a
        else:
            if a.numel() and (a.is_floating_point() or a.is_complex()):
                raise ValueError("allowed_codes: a bool [n_class] mask or a collection of integer class indices")
            a = a.reshape(-1).long()
            if a.numel() and (int(a.min()) < 0 or int(a.max()) >= n):
                raise ValueError(f"allowed_codes: class indices lie in [0, {n})")
            allowed = torch.zeros(n, dtype=torch.bool)
            allowed[a] = True
        table = torch.full((1, n), -float("inf"), dtype=torch.float32)
        table[0, allowed] = 0.0
    else:
        if not torch.is_tensor(code_bias) or not code_bias.is_floating_point():
            raise ValueError("code_bias: a float tensor [n_class] or [R, n_class]")
        table = code_bias.detach().to(device="cpu", dtype=torch.float32)
        if table.dim() == 1:
            table = table.unsqueeze(0)
        if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != n:
            raise ValueError(f"code_bias {tuple(code_bias.shape)}: expected [{n}] or [R, {n}] (n_class_target)")
        if table.shape[0] > 1 and code_bias_map is None:
            raise ValueError(f"code_bias with {table.shape[0]} rows needs a code_bias_map to choose among them")
    if bool(torch.isnan(table).any()) or bool((table == float("inf")).any()):
        raise ValueError("code_bias: NaN and +inf are not biases (-inf bans a class)")
    if not bool(torch.isfinite(table).any(dim=1).all()):
        raise ValueError("code_bias / allowed_codes: a row that bans every class")
    if code_bias_map is None:
        return table.contiguous(), None
    helper = model.target_codemaps_helper
    m = code_bias_map
    if not torch.is_tensor(m) or m.is_floating_point() or m.is_complex() or m.dtype == torch.bool:
        raise ValueError("code_bias_map: an integer tensor [F, T], [1, F, T] or [B, F, T]; -1 = no bias")
    m = m.detach().cpu().long()
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if m.dim() != 3 or tuple(m.shape[1:]) != (helper.frequencies, helper.duration) or m.shape[0] not in (1, batch_size):
        raise ValueError(f"code_bias_map {tuple(code_bias_map.shape)}: expected [{helper.frequencies}, {helper.duration}] with "
                         f"no, 1 or {batch_size} leading rows")
    if int(m.max()) >= table.shape[0]:
        raise ValueError(f"code_bias_map: index {int(m.max())} into a table of {table.shape[0]} rows")
    return table.contiguous(), m.clamp(min=-1)


def _code_bias_index(model, bias_map) -> torch.Tensor:
    """int32 [1 or B, S]: a checked map of bias rows in the order the loop samples in (the mask's way into that order)."""
    if bias_map is None:
        return torch.zeros(1, model.target_transformer_sequence_length, dtype=torch.int32)
    return model.target_codemaps_helper.to_sequence(bias_map).to(torch.int32).contiguous()


@torch.no_grad()
def sample_model(model: VQNSynthTransformer, device: Union[torch.device, str], batch_size: int,
                 codemap_size: Iterable[int], temperature: Union[float, Sequence[float], torch.Tensor],
                 condition: Optional[torch.Tensor] = None, constraint: Optional[torch.Tensor] = None,
                 class_conditioning: Mapping[str, Iterable[int]] = {},
                 initial_code: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                 local_class_conditioning_map=None,
                 time_indexes_source: Optional[Iterable[int]] = None,
                 time_indexes_target: Optional[Iterable[int]] = None,
                 top_k_sampling_k: Union[int, Sequence[int], torch.Tensor] = 0,
                 top_p_sampling_p: Union[float, Sequence[float], torch.Tensor] = 0.0,
                 progressbar_decorator=None, use_predictive_sampling: bool = False,
                 generator: Optional[torch.Generator] = None,
                 uniforms: Optional[torch.Tensor] = None,
                 gumbel_noise: Optional[torch.Tensor] = None,
                 kv_cache_dtype: Optional[torch.dtype] = None,
                 num_variations: Optional[int] = None, return_log_probs: bool = False,
                 code_bias: Optional[torch.Tensor] = None, code_bias_map: Optional[torch.Tensor] = None,
                 allowed_codes=None):
    """code_bias / code_bias_map / allowed_codes: steer WHAT may be drawn, per codemap cell.  `code_bias` is a float tensor
    [n_class] added to the logits of every sampled cell before temperature and filters, or a table [R, n_class] together
    with `code_bias_map`, an integer tensor [F, T], [1, F, T] or [B, F, T] in codemap layout naming the table row of every
    cell (-1: no bias there).  -inf bans a class -- it is never drawn; NaN, +inf and a row that bans every class are
    refused.  `allowed_codes` (a bool [n_class], e.g. `codes_in_use(...)`, or a collection of class indices) is shorthand
    for one row of 0 and -inf.  The draw kernel adds the row (`isi_prior_code_bias`); log-probabilities reported with
    `return_log_probs` stay the MODEL's.  With the options off the call is what it was.
    return_log_probs: the result is (codes [B, F, T], log_probs [B, F, T] float32) -- beside every sampled code the
    MODEL's log-probability of it (log softmax of the raw logits: it does not depend on temperature, top-k or top-p, and it
    is what `score_codemap` gives for the result), exactly 0.0 where nothing was sampled.  The draw kernel stores it as it
    commits the token (`isi_prior_state.token_log_probs`); the codes are those of the call without the option.
    num_variations: N alternatives for ONE request -- `batch_size` is 1 and condition, initial code, mask and class
    conditioning are that request's; the result is [N, F, T], row n drawn with `uniforms[:, n]` ([S, N], from `generator`
    when not given).  The source sequence, the encoder and the prefix pass run once at batch 1 and every row reads one copy
    of the projected memory (`_sample_variations`).  The codes are those of `batch_size=N` with the inputs repeated N times.
    kv_cache_dtype: format of the loop's two key/value caches -- torch.float32, torch.bfloat16, or None for the switch
    ISI_DECODE_KV (f32 | bf16, default f32).  Predictive sampling runs full passes and has no cache.
    Ragged batches: rows are independent requests.  `mask` [B, F, T] may differ per row (each row walks its own span),
    `time_indexes_source` / `time_indexes_target` may be [B, T] tensors, and `temperature`, `top_k_sampling_k`,
    `top_p_sampling_p` may be length-B sequences or tensors.  A [1, F, T] mask or one whose rows are all equal, with
    shared parameters, samples exactly as a single request does."""
    if constraint is not None:
        raise NotImplementedError
    if return_log_probs and use_predictive_sampling:
        raise ValueError("return_log_probs reads the KV-cached loop's draw kernel: predictive sampling draws by Gumbel-max "
                         "over full passes and reports no log-probabilities")
    bias_table, bias_map = _code_bias_rows(model, batch_size, code_bias, code_bias_map, allowed_codes)
    bias_index = _code_bias_index(model, bias_map) if bias_table is not None else None
    if bias_table is not None and use_predictive_sampling:
        raise ValueError("code_bias / allowed_codes are applied by the KV-cached loop's draw kernel: predictive sampling "
                         "draws by Gumbel-max over full passes")
    if num_variations is not None:
        return _sample_variations(model, device, batch_size, codemap_size, temperature, condition, class_conditioning,
                                  initial_code, mask, time_indexes_source, time_indexes_target, top_k_sampling_k,
                                  top_p_sampling_p, progressbar_decorator, use_predictive_sampling, generator, uniforms,
                                  kv_cache_dtype, num_variations, return_log_probs, bias_table, bias_index)
    kv_cache_dtype = _kv_cache_dtype(kv_cache_dtype)
    if use_predictive_sampling and kv_cache_dtype is not torch.float32:
        raise ValueError("predictive sampling runs full decoder passes and has no key/value cache: kv_cache_dtype / "
                         "ISI_DECODE_KV do not apply")
    device = torch.device(device)
    if mask is not None and mask.dim() == 3 and mask.shape[0] not in (1, batch_size):
        raise ValueError(f"mask for {mask.shape[0]} rows, batch of {batch_size}")
    rows_differ = (mask is not None and mask.dim() == 3 and mask.shape[0] > 1 and
                   not bool((mask == mask[:1]).all()))
    if use_predictive_sampling and rows_differ:
        raise ValueError("predictive sampling decodes every row at the same positions: the rows' masks must be equal")
    row_params = [_per_row(v, batch_size, n) for v, n in ((temperature, "temperature"), (top_k_sampling_k, "top_k_sampling_k"),
                                                        (top_p_sampling_p, "top_p_sampling_p"))]
    if use_predictive_sampling and any(t is not None for _, t in row_params):
        raise ValueError("predictive sampling takes one temperature / top-k / top-p for all rows")
    model.eval()
    if batch_size > 256:
        # the native loop decodes up to 256 sequences at a time: larger requests run chunk by chunk (rows are
        # independent; every chunk gets its own slice of the per-row inputs and of the uniforms)
        if uniforms is None:
            uniforms = torch.rand(model.target_transformer_sequence_length, batch_size, generator=generator)

        def rows(t, lo, hi):
            if t is None or not torch.is_tensor(t) or t.dim() == 0 or t.shape[0] != batch_size:
                return t
            return t[lo:hi]

        def param_rows(v, lo, hi):           # a per-row sampling parameter (else the shared value)
            return v[1][lo:hi] if v[1] is not None else v[0]

        def time_rows(ti, lo, hi):           # [B, T] per-row time indexes (a 1-D list is shared)
            return ti[lo:hi] if torch.is_tensor(ti) and ti.dim() == 2 else ti

        def bias_map_rows(lo, hi):           # the checked table goes through as it is; a per-row map is sliced
            return bias_map[lo:hi] if bias_map is not None and bias_map.shape[0] > 1 else bias_map

        parts = []
        for lo in range(0, batch_size, 256):
            hi = min(batch_size, lo + 256)
            cls = {k: (torch.as_tensor(v).reshape(-1)[lo:hi] if torch.as_tensor(v).numel() == batch_size else v)
                   for k, v in class_conditioning.items()}
            # every per-row input is sliced (a mask with a batch dimension included); options are passed through
            parts.append(sample_model(
                model, device, hi - lo, codemap_size, param_rows(row_params[0], lo, hi), condition=rows(condition, lo, hi),
                class_conditioning=cls, initial_code=rows(initial_code, lo, hi), mask=rows(mask, lo, hi),
                time_indexes_source=time_rows(time_indexes_source, lo, hi),
                time_indexes_target=time_rows(time_indexes_target, lo, hi),
                top_k_sampling_k=param_rows(row_params[1], lo, hi), top_p_sampling_p=param_rows(row_params[2], lo, hi),
                progressbar_decorator=progressbar_decorator, use_predictive_sampling=use_predictive_sampling,
                uniforms=uniforms[:, lo:hi], gumbel_noise=rows(gumbel_noise, lo, hi), kv_cache_dtype=kv_cache_dtype,
                return_log_probs=return_log_probs, code_bias=bias_table, code_bias_map=bias_map_rows(lo, hi)))
        if return_log_probs:
            return torch.cat([c for c, _ in parts], 0), torch.cat([lp for _, lp in parts], 0)
        return torch.cat(parts, 0)
    if initial_code is None:
        fill = model.mask_token_index if model.self_conditional_model else 0
        codemap = torch.full([batch_size] + list(codemap_size), fill, dtype=torch.int64, device=device)
    else:
        codemap = initial_code.to(device)
    cls = {}
    for name, value in class_conditioning.items():
        value = torch.as_tensor(value).long().reshape(-1)
        cls[name] = (value.expand(batch_size) if value.numel() == 1 else value).reshape(batch_size, 1).to(device)
    if model.self_conditional_model:
        condition = codemap
    if mask is not None:
        mask = mask.to(device)
    # With no initial_code the reference fills the map with the mask token, which its
    # target embedding cannot index (sample.py:167-171 vs priors/transformer.py:286: an
    # IndexError there).  Those target rows are always overwritten by samples before the
    # decoder reads them, so the target side is built from in-range placeholders.
    target_codemap = codemap.clamp(max=model.n_class_target - 1) if initial_code is None else codemap
    source_seq, target_seq = model.to_sequences(
        target_codemap, condition.to(device), class_conditioning=cls, mask=mask,
        time_indexes_source=time_indexes_source, time_indexes_target=time_indexes_target)

    S = model.target_transformer_sequence_length
    start_len = model.target_start_symbol.shape[1]
    code_seq = model.target_codemaps_helper.to_sequence(codemap).clone()
    (temperature, temp_rows), (top_k_sampling_k, top_k_rows), (top_p_sampling_p, top_p_rows) = row_params
    mask_rows = None
    if mask is not None:
        mseq = model.target_codemaps_helper.to_sequence(mask).reshape(-1, S).cpu().numpy()
        mask_seq = mseq[0]
        if rows_differ:
            mask_rows = mseq
    else:
        mask_seq = [True] * S
    ragged = mask_rows is not None or any(t is not None for t in (temp_rows, top_k_rows, top_p_rows))
    if ragged and mask_rows is None:
        mask_rows = np.broadcast_to(np.asarray(mask_seq, dtype=bool), (batch_size, S))
    if use_predictive_sampling:
        return _predictive_sampling(model, source_seq, target_seq, code_seq, mask_seq, start_len, temperature,
                                    top_k_sampling_k, top_p_sampling_p, gumbel_noise, progressbar_decorator)
    if uniforms is None:
        uniforms = torch.rand(S, batch_size, generator=generator)
    uniforms = uniforms.to(device=device, dtype=torch.float32)

    # encoder memory once (anti-causal for the self-conditional top prior)
    src = source_seq.transpose(0, 1).contiguous()
    memory, *_ = model.transformer.encoder(src, mask='anticausal' if model.self_conditional_model else None)
    x_seq = target_seq.transpose(0, 1).contiguous()          # [S_t, B, d]; rows are rewritten as we sample
    if not code_seq.is_contiguous():
        code_seq = code_seq.contiguous()
    if ragged:
        # independent requests: every row walks its own span (isi_prior_sample_run_rows); one causal prefill covers every
        # row's unmasked prefix -- slots it fills beyond a row's own first position are rewritten by that row's steps
        # before any later position reads them
        pos, commit, p0 = _ragged_plan(np.asarray(mask_rows, dtype=bool), start_len - 1)
        if pos.shape[0] == 0:
            return _maps(model, code_seq, return_log_probs, None)
        sampler = NativeSampler(model, memory, x_seq, code_seq, mask_seq, uniforms, kv_cache_dtype=kv_cache_dtype,
                                log_probs=return_log_probs, code_bias=bias_table, code_bias_index=bias_index)
        n_steps = sampler.plan_rows(pos, commit, temp_rows, top_k_rows, top_p_rows)
        sampler.prefill(p0)
        chunk = n_steps if progressbar_decorator is None else 64
        starts = range(0, n_steps, chunk)
        if progressbar_decorator is not None:
            starts = progressbar_decorator(starts)
        for t0 in starts:
            sampler.run_rows(t0, min(n_steps, t0 + chunk), temperature, top_k_sampling_k, top_p_sampling_p)
        return _maps(model, code_seq, return_log_probs, sampler.log_probs)
    n_pos = S + start_len - 1
    # Token i is drawn from decoder position i + start_len - 1.  Positions behind the last masked token are
    # never read; positions before the first one only contribute keys / values, which one batched causal
    # pass over that prefix provides (an inpainting request masks a window, not the whole map).
    masked = [i for i, mk in enumerate(mask_seq) if mk]
    if not masked:
        return _maps(model, code_seq, return_log_probs, None)
    p_first, n_pos = masked[0] + start_len - 1, min(n_pos, masked[-1] + start_len)
    # the whole loop natively: no per-token return to Python, no host sync
    sampler = NativeSampler(model, memory, x_seq, code_seq, mask_seq, uniforms, kv_cache_dtype=kv_cache_dtype,
                            log_probs=return_log_probs, code_bias=bias_table, code_bias_index=bias_index)
    if p_first < 8:
        p_first = 0                                        # a few rows: not worth a batched pass
    sampler.prefill(p_first)
    chunk = n_pos if progressbar_decorator is None else 64
    starts = range(p_first, n_pos, chunk)
    if progressbar_decorator is not None:
        starts = progressbar_decorator(starts)
    for p0 in starts:
        sampler.run(p0, min(n_pos, p0 + chunk), temperature, top_k_sampling_k, top_p_sampling_p)
    return _maps(model, code_seq, return_log_probs, sampler.log_probs)


def _maps(model, code_seq, return_log_probs: bool, log_probs: Optional[torch.Tensor]):
    """The sampled sequences as codemaps: codes [B, F, T], and with `return_log_probs` the tokens' log-probabilities in the
    same layout (all zero when nothing was sampled)."""
    codes = model.target_codemaps_helper.to_time_frequency_map(code_seq).long()
    if not return_log_probs:
        return codes
    if log_probs is None:
        log_probs = torch.zeros(code_seq.shape, dtype=torch.float32, device=code_seq.device)
    return codes, model.target_codemaps_helper.to_time_frequency_map(log_probs)


@torch.no_grad()
def score_codemap(model: VQNSynthTransformer, device: Union[torch.device, str], codemap: torch.Tensor,
                  condition: Optional[torch.Tensor] = None, class_conditioning: Mapping[str, Iterable[int]] = {},
                  mask: Optional[torch.Tensor] = None, time_indexes_source: Optional[Iterable[int]] = None,
                  time_indexes_target: Optional[Iterable[int]] = None) -> torch.Tensor:
    """float32 [B, F, T]: the model's log-probability of every code of `codemap` [B, F, T] given the codes before it (in
    the target helper's order) and the source -- a sampled map, an edited one, or one encoded from audio.  ONE teacher-forced
    full pass: the sequences are built by `model.to_sequences` exactly as `sample_model` builds them, the forward kernels
    give the logits of all B S rows and `isi_token_log_prob_f32` reads the codes' entries of their log softmax.
    condition: the source codemap (the top codes for a bottom prior); a self-conditional model may leave it out (the
    codemap itself).  mask: `sample_model`'s inpainting mask -- it hides the source side as it did when sampling, and
    positions outside it are 0.0.  For a result c of `sample_model(..., initial_code=i, condition=x, mask=m)`,
    `score_codemap(model, device, c, condition=(i if model.self_conditional_model else x), mask=m)` with the same
    conditioning reproduces the loop's `return_log_probs`."""
    logits, code_seq, mask_seq = _teacher_forced_logits("score_codemap", model, device, codemap, condition,
                                                        class_conditioning, mask, time_indexes_source, time_indexes_target)
    log_probs = _ops.token_log_probs(logits, code_seq)                         # [B, S]
    if mask_seq is not None:
        log_probs = torch.where(mask_seq, log_probs, torch.zeros((), dtype=torch.float32, device=logits.device))
    return model.target_codemaps_helper.to_time_frequency_map(log_probs)


def _teacher_forced_logits(who: str, model, device, codemap, condition, class_conditioning, mask, time_indexes_source,
                           time_indexes_target):
    """The one teacher-forced full pass behind `score_codemap` and `codemap_statistics`: (logits [B, S, n_class] contiguous,
    the codemap as sequences [B, S] int64, the mask as sequences [B or 1, S] bool or None)."""
    device = torch.device(device)
    model.eval()
    codemap = codemap.to(device)
    batch_size = codemap.shape[0]
    if condition is None:
        if not model.self_conditional_model:
            raise ValueError(f"{who}: a model that is not self-conditional needs its condition codemap")
        condition = codemap
    if mask is not None:
        if mask.dim() == 3 and mask.shape[0] not in (1, batch_size):
            raise ValueError(f"mask for {mask.shape[0]} rows, batch of {batch_size}")
        mask = mask.to(device)
    cls = {}
    for name, value in class_conditioning.items():
        value = torch.as_tensor(value).long().reshape(-1)
        cls[name] = (value.expand(batch_size) if value.numel() == 1 else value).reshape(batch_size, 1).to(device)
    source_seq, target_seq = model.to_sequences(
        codemap, condition.to(device), class_conditioning=cls, mask=mask,
        time_indexes_source=time_indexes_source, time_indexes_target=time_indexes_target)
    logits, _ = model(target_seq, source_seq)                                  # [B, S, n_class]
    code_seq = model.target_codemaps_helper.to_sequence(codemap).contiguous()
    mask_seq = None
    if mask is not None:
        S = model.target_transformer_sequence_length
        mask_seq = model.target_codemaps_helper.to_sequence(mask).reshape(-1, S)
    return logits.contiguous(), code_seq, mask_seq


class CodemapStatistics(NamedTuple):
    """`codemap_statistics`' maps, [B, F, T] each (the top-n maps [B, F, T, top_n])."""
    log_probs: torch.Tensor
    entropy: torch.Tensor
    rank: torch.Tensor
    top_codes: torch.Tensor
    top_log_probs: torch.Tensor


@torch.no_grad()
def codemap_statistics(model: VQNSynthTransformer, device: Union[torch.device, str], codemap: torch.Tensor,
                       condition: Optional[torch.Tensor] = None, class_conditioning: Mapping[str, Iterable[int]] = {},
                       mask: Optional[torch.Tensor] = None, time_indexes_source: Optional[Iterable[int]] = None,
                       time_indexes_target: Optional[Iterable[int]] = None, top_n: int = 0) -> CodemapStatistics:
    """What the model thinks of every code of `codemap` [B, F, T], from `score_codemap`'s single teacher-forced pass (the
    same arguments, the same logits) and one `isi_token_stats_f32` call over its B S rows:
      log_probs      float32 [B, F, T]: `score_codemap`'s result, bit for bit;
      entropy        float32 [B, F, T]: the entropy in nats of the model's distribution at the position (raw logits,
                     temperature 1, nothing filtered) -- high: the model is unsure; low with a low log-probability: the code
                     surprises it;
      rank           int32 [B, F, T]: how many classes the model ranks ahead of the code that is there (0: its first choice);
      top_codes      int64 [B, F, T, top_n] and top_log_probs float32 [B, F, T, top_n]: the model's top_n (0 .. 16) classes
                     for the position, most likely first (equal logits: lower class first), and their log-probabilities.
    Outside `mask`: log_probs 0.0, entropy 0.0, rank -1, top_codes -1, top_log_probs -inf.
    The values are teacher-forced: the decoder is causal, so position i is scored given the codes of `codemap` before it,
    as the sampling loop saw them.  The SOURCE side is different: a self-conditional prior scored WITHOUT a mask reads the
    whole codemap through its encoder, the scored position included -- its statistics are then those of a model that
    already knows the answer (log-probabilities near 0, entropies near 0, ranks 0).  To ask what the model would put in a
    region, pass the region as `mask`: the encoder then sees mask tokens there, as it did when sampling."""
    if not 0 <= int(top_n) <= 16:
        raise ValueError(f"codemap_statistics: top_n must be 0 .. 16, not {top_n}")
    logits, code_seq, mask_seq = _teacher_forced_logits("codemap_statistics", model, device, codemap, condition,
                                                        class_conditioning, mask, time_indexes_source, time_indexes_target)
    st = _ops.token_stats(logits, code_seq, int(top_n))
    top_codes, top_log_probs = st.top_codes, st.top_log_probs
    if top_codes is None:
        top_codes = torch.empty(code_seq.shape + (0,), dtype=torch.int64, device=logits.device)
        top_log_probs = torch.empty(code_seq.shape + (0,), dtype=torch.float32, device=logits.device)
    maps = [st.log_probs, st.entropy, st.rank, top_codes, top_log_probs]
    if mask_seq is not None:
        outside = (0.0, 0.0, -1, -1, float("-inf"))
        maps = [torch.where(mask_seq if t.dim() == 2 else mask_seq[..., None], t,
                            torch.full((), v, dtype=t.dtype, device=t.device)) for t, v in zip(maps, outside)]
    return CodemapStatistics(*(model.target_codemaps_helper.to_time_frequency_map(t) for t in maps))


def _one_value(value, name: str):
    """A sampling parameter of variations mode: one value for all rows (a scalar, or equal entries)."""
    if torch.is_tensor(value) or isinstance(value, (list, tuple, np.ndarray)):
        t = torch.as_tensor(value).reshape(-1).cpu()
        if t.numel() == 0 or not bool((t == t[0]).all()):
            raise ValueError(f"num_variations: {name} is one value for all variations (rows of one request), not per row")
        return t[0].item()
    return value


def _sample_variations(model, device, batch_size, codemap_size, temperature, condition, class_conditioning, initial_code,
                       mask, time_indexes_source, time_indexes_target, top_k, top_p, progressbar_decorator,
                       use_predictive_sampling, generator, uniforms, kv_cache_dtype, num_variations,
                       return_log_probs=False, bias_table=None, bias_index=None):
    """`sample_model(num_variations=N)`: N rows over ONE source.  Everything that does not depend on the draws is formed once at
    batch 1 -- source sequence, encoder memory, its projected keys / values (or the single-source table) and the keys / values
    of the unmasked prefix; the target rows, the codes and the self-attention cache have N rows.  All checks come before any
    device work."""
    N = int(num_variations)
    if N < 1:
        raise ValueError(f"num_variations must be at least 1, not {num_variations}")
    if use_predictive_sampling:
        raise ValueError("num_variations runs the KV-cached loop: use_predictive_sampling does not apply")
    if batch_size != 1:
        raise ValueError(f"num_variations samples N rows of ONE request: batch_size must be 1, not {batch_size}")
    for name, t in (("condition", condition), ("initial_code", initial_code)):
        if t is not None and t.shape[0] != 1:
            raise ValueError(f"num_variations: {name} is one request's ([1, ...]), not {tuple(t.shape)}")
    if mask is not None and mask.dim() == 3 and mask.shape[0] != 1:
        if not bool((mask == mask[:1]).all()):
            raise ValueError("num_variations: the rows are variations of one request, their masks cannot differ")
        mask = mask[:1]
    for name, ti in (("time_indexes_source", time_indexes_source), ("time_indexes_target", time_indexes_target)):
        if torch.is_tensor(ti) and ti.dim() == 2 and ti.shape[0] != 1:
            raise ValueError(f"num_variations: {name} is one request's, not {tuple(ti.shape)}")
    for name, value in class_conditioning.items():
        if torch.as_tensor(value).numel() != 1:
            raise ValueError(f"num_variations: class_conditioning[{name!r}] is one request's value")
    temperature = _one_value(temperature, "temperature")
    top_k, top_p = _one_value(top_k, "top_k_sampling_k"), _one_value(top_p, "top_p_sampling_p")
    kv_cache_dtype = _kv_cache_dtype(kv_cache_dtype)
    S = model.target_transformer_sequence_length
    if uniforms is not None and tuple(uniforms.shape) != (S, N):
        raise ValueError(f"num_variations: uniforms are [S, N] = [{S}, {N}], not {tuple(uniforms.shape)}")
    device = torch.device(device)
    model.eval()
    if uniforms is None:
        uniforms = torch.rand(S, N, generator=generator)
    if initial_code is None:
        fill = model.mask_token_index if model.self_conditional_model else 0
        codemap = torch.full([1] + list(codemap_size), fill, dtype=torch.int64, device=device)
    else:
        codemap = initial_code.to(device)
    cls = {name: torch.as_tensor(value).long().reshape(1, 1).to(device) for name, value in class_conditioning.items()}
    if model.self_conditional_model:
        condition = codemap
    if mask is not None:
        mask = mask.to(device)
    target_codemap = codemap.clamp(max=model.n_class_target - 1) if initial_code is None else codemap
    source_seq, target_seq = model.to_sequences(
        target_codemap, condition.to(device), class_conditioning=cls, mask=mask,
        time_indexes_source=time_indexes_source, time_indexes_target=time_indexes_target)
    start_len = model.target_start_symbol.shape[1]
    code_row = model.target_codemaps_helper.to_sequence(codemap)                           # [1, S]
    mask_seq = (model.target_codemaps_helper.to_sequence(mask).reshape(-1, S).cpu().numpy()[0] if mask is not None
                else [True] * S)
    masked = [i for i, mk in enumerate(mask_seq) if mk]
    if not masked:
        return _maps(model, code_row.repeat(N, 1).contiguous(), return_log_probs, None)
    # one encoder pass for all variations (anti-causal for the self-conditional top prior)
    memory, *_ = model.transformer.encoder(source_seq.transpose(0, 1).contiguous(),
                                           mask='anticausal' if model.self_conditional_model else None)
    x_row = target_seq.transpose(0, 1).contiguous()                                        # [S_t, 1, d]
    p_first, n_pos = masked[0] + start_len - 1, min(S + start_len - 1, masked[-1] + start_len)
    if p_first < 8:
        p_first = 0
    parts = []
    for lo in range(0, N, 256):                    # the native loop decodes up to 256 rows at a time
        n = min(N, lo + 256) - lo
        x_seq = x_row.repeat(1, n, 1).contiguous()
        code_seq = code_row.repeat(n, 1).contiguous()
        sampler = NativeSampler(model, memory, x_seq, code_seq, mask_seq, uniforms[:, lo:lo + n].to(device=device, dtype=torch.float32),
                                kv_cache_dtype=kv_cache_dtype, shared_memory=True, log_probs=return_log_probs,
                                code_bias=bias_table, code_bias_index=bias_index)
        sampler.prefill(p_first)
        chunk = n_pos if progressbar_decorator is None else 64
        starts = range(p_first, n_pos, chunk)
        if progressbar_decorator is not None:
            starts = progressbar_decorator(starts)
        for p0 in starts:
            sampler.run(p0, min(n_pos, p0 + chunk), temperature, top_k, top_p)
        parts.append(_maps(model, code_seq, return_log_probs, sampler.log_probs))
    if return_log_probs:
        return torch.cat([c for c, _ in parts], 0), torch.cat([lp for _, lp in parts], 0)
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def _predictive_sampling(model, source_seq, target_seq, code_seq, mask_seq, start_len, temperature, top_k, top_p,
                         gumbel_noise, progressbar_decorator):
    """Predictive sampling of the reference (sample.py:251-261,268-342): with the Gumbel reparametrisation
    `argmax(log p + g)` and the noise `g` drawn up front, every full pass also FORECASTS all later masked tokens; a
    step whose forecast already equalled the token the previous pass put there is skipped.  The sampled map is that of
    sequential Gumbel-max sampling with the same noise.  One full decoder pass per non-skipped step (the encoder
    memory is cached), on the HIP forward kernels; the KV-cached loop does not apply -- a pass rewrites every later
    input row.  Differences from the reference: its boolean index `[1, S]` on `[B, S]` tensors only works at batch 1,
    here the mask broadcasts over the batch; `gumbel_noise` ([B, S, n_class]) may be passed in (tests)."""
    device = target_seq.device
    B, S = code_seq.shape
    eff = model.embeddings_effective_dim
    if gumbel_noise is None:
        gumbel_noise = torch.distributions.gumbel.Gumbel(torch.zeros(B, S, model.n_class_target), 1).sample()
    gumbel_noise = gumbel_noise.to(device=device, dtype=torch.float32)
    mask_t = torch.as_tensor(list(mask_seq), dtype=torch.bool, device=device)          # [S]
    positions = torch.arange(S, device=device)
    source_start = model.source_start_symbol.shape[1] if hasattr(model, "source_start_symbol") else start_len
    memory = None
    sample = None
    prediction_was_correct = False
    correct_predictions = 0
    previous = code_seq
    steps = enumerate(mask_seq)
    if progressbar_decorator is not None:
        steps = progressbar_decorator(steps)
    for i, is_masked in steps:
        if not is_masked:
            continue
        if sample is not None and prediction_was_correct:
            prediction_was_correct = bool(torch.all(sample[:, i] == previous[:, i]))
            if prediction_was_correct:
                correct_predictions += 1
                continue
        logits, memory = model(target_seq, source_seq, memory=memory)
        logits = top_k_top_p_filtering(logits / temperature, top_k=top_k, top_p=top_p)
        probabilities = torch.softmax(logits, dim=-1)
        sample = torch.argmax(torch.log(probabilities) + gumbel_noise, dim=-1)        # [B, S]
        prediction_was_correct = bool(torch.all(sample[:, i] == code_seq[:, i]))
        previous = code_seq.clone()
        update = (mask_t & (positions >= i)).unsqueeze(0).expand(B, S)                 # causal and inpainting mask
        code_seq[update] = sample[update]
        embedded = model.embed_data(sample, Seq2SeqInputKind.Target)                   # [B, S, eff]
        tgt_view = target_seq[:, start_len:, :eff]
        tgt_view[update] = embedded[update]
        if model.self_conditional_model:
            src_view = source_seq[:, source_start:, :eff]
            src_view[update] = embedded[update]
            # the cached memory stays valid: the top encoder's attention is anti-causal (reference comment)
    model.predictive_sampling_correct_ratio = correct_predictions / max(1, len(mask_seq))
    return model.target_codemaps_helper.to_time_frequency_map(code_seq).long()
