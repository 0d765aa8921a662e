"""Interactive inpainting operations on MI355X: the compute behind the reference's Flask
routes (flask_server.py), free of HTTP so that they can be called, tested and timed directly.

  make_time_indexes   positional-embedding time indexes of a model window inside a longer
                      codemap (flask_server.py:670-682)
  timerange_change    regenerate the masked zone of the top (and then bottom) or of the bottom
                      codemap inside the window starting at `start_index_top`
                      (flask_server.py:685-870)
  timerange_change_batch   independent timerange_change requests in one ragged top and one ragged bottom call
  erase               attenuate the log-magnitude under the mask and re-encode (:873-931)
  generate            new top + bottom codemaps from scratch (:376-443)
  codes_to_audio      VQ-VAE decode + spectrogram inversion (:1003-1021)
  top_conditioned_sample / analyze_audio    (:1049-1110 / :624-667)
  sample_from_database   a stored (top, bottom) pair whose attributes meet the request's constraints,
                      cut / padded to the requested duration (:314-372, 446-514); optionally the one nearest to a sound
  similar_sounds      the stored sounds most like a given one, optionally outside a masked region (not in the
                      reference: utils/datasets/code_index.py, csrc/code_search.hip)
  similar_sounds_to_spectrogram / similar_fragments_to_spectrogram / similar_to_mixture   the same questions for a sound
                      that is no codemap -- an upload's encoder vectors, a morph's blends -- compared with the stored
                      codes' vectors without snapping it to codes first (CodeIndex.search_soft)
  morph / morph_sweep / crossfade   decode per-cell weighted mixtures of several sounds' codes: timbre interpolation,
                      a sweep between two sounds in one batch, a splice whose seam is a ramp in the latent (not in the
                      reference: csrc/code_mix.hip, VQVAE.decode_code_mix)
  codes_to_audio_spliced / splice_weights / changed_cells   `codes_to_audio` for an UPLOAD whose codes were edited: the
                      upload's own samples outside the edit, the decoded codes inside it, phase-locked at both seams
                      (not in the reference: csrc/spec_splice.hip, SpectrogramsHelper.to_audio_spliced)
  stretch_sound / transpose_sound   a sound (or decoded codes) at another length, a sound at another pitch -- by a number
                      of semitones, to a MIDI pitch, or to the estimated pitch of another sound -- with its codes, so that
                      morphs and searches can compare sounds at equal pitch (not in the reference: csrc/stft_stretch.hip,
                      GANsynth_pytorch/stretch.py); `preserve_formants=True` there and on `bend_sound` leaves the
                      resonances where they were (csrc/formant.hip)
  shift_formants_sound   a sound at its own pitch with its formants moved, with its codes
  spectrogram_png     the decoded log-mel magnitude as a viridis PNG (:103-143, 1024-1046)

The heavy work is `sample.sample_model` (encoder pass + KV-cached native decoding loop),
`VQVAE.decode_code / encode` and `SpectrogramsHelper.to_audio`: all HIP kernels.
"""
from __future__ import annotations

import inspect
import math
import struct
import zlib
from types import SimpleNamespace
from typing import List, Mapping, Optional, Sequence, Tuple

import torch

from sample import _code_bias_rows, codemap_statistics, sample_model


def make_time_indexes(start_index: int, codemap_duration: int, transformer_duration: int) -> List[int]:
    """Index 0 marks the attack, index `transformer_duration - 1` the release; the frames in between
    share the remaining `transformer_duration - 2` indexes in equal runs (the last index takes the
    remainder).  Returns the slice seen by a window starting at `start_index`."""
    inner = transformer_duration - 2           # indexes 1 .. inner available for the sustain
    frames = codemap_duration - 2              # frames to label with them
    run = frames // inner
    full = [0]
    for i in range(1, inner):
        full += [i] * run
    full += [inner] * (frames - (len(full) - 1))
    full.append(transformer_duration - 1)
    return full[start_index:start_index + transformer_duration]


def _windows(top_code, bottom_code, transformer_top, transformer_bottom, start_index_top):
    ratio_t = transformer_bottom.shape[1] // transformer_top.shape[1]
    s_top, e_top = start_index_top, start_index_top + transformer_top.shape[1]
    s_bot = ratio_t * start_index_top
    e_bot = s_bot + transformer_bottom.shape[1]
    return (s_top, e_top), (s_bot, e_bot), ratio_t


def _check_score_options(return_scores, sort_by_likelihood, uniform_sampling) -> None:
    """The combinations of `timerange_change`'s score options that have no meaning (ValueError)."""
    if sort_by_likelihood and not return_scores:
        raise ValueError("sort_by_likelihood orders the variations by their scores: it needs return_scores=True")
    if return_scores and uniform_sampling:
        raise ValueError("return_scores: uniform_sampling draws from no model distribution, there is no likelihood to report")


# Per-layer steering of what may be drawn (`sample_model`'s allowed_codes / code_bias / code_bias_map): a request changes up to
# two layers, each with its own classes, so the options are given per layer -- allowed_codes_top, code_bias_bottom, ... --
# with code_bias_map_* [F, W] or [1, F, W] over the model window in that layer's resolution.
_CODE_BIAS_OPTIONS = ('allowed_codes', 'code_bias', 'code_bias_map')
_CODE_BIAS_KEYWORDS = frozenset(f"{name}_{layer}" for name in _CODE_BIAS_OPTIONS for layer in ('top', 'bottom'))


def _split_code_bias(kwargs: Mapping, uniform_sampling: bool = False):
    """(the other keywords, {'top': sample_model's options for the top prior, 'bottom': ...}) of a keyword mapping."""
    plain = set(kwargs) & set(_CODE_BIAS_OPTIONS)
    if plain:
        raise TypeError(f"{sorted(plain)}: the two layers have their own classes -- give "
                        f"{', '.join(sorted(f'{n}_top / {n}_bottom' for n in plain))}")
    rest = {k: v for k, v in kwargs.items() if k not in _CODE_BIAS_KEYWORDS}
    bias = {layer: {name: kwargs[f"{name}_{layer}"] for name in _CODE_BIAS_OPTIONS if kwargs.get(f"{name}_{layer}") is not None}
            for layer in ('top', 'bottom')}
    if uniform_sampling and (bias['top'] or bias['bottom']):
        raise ValueError("uniform_sampling draws from no model distribution: allowed_codes / code_bias do not apply")
    return rest, bias


@torch.no_grad()
def timerange_change(transformer_top, transformer_bottom, top_code: torch.Tensor, bottom_code: torch.Tensor,
                     mask: torch.Tensor, layer: str, start_index_top: int, temperature: float,
                     class_conditioning_top: Mapping[str, torch.Tensor],
                     class_conditioning_bottom: Mapping[str, torch.Tensor], device,
                     uniform_sampling: bool = False, generator: Optional[torch.Generator] = None,
                     kv_cache_dtype: Optional[torch.dtype] = None, num_variations: Optional[int] = None,
                     return_scores: bool = False, sort_by_likelihood: bool = False,
                     **sampling_kwargs) -> Tuple[torch.Tensor, ...]:
    """top_code [1,F_t,T], bottom_code [1,F_b,T_b] (T may exceed the models' duration), mask bool
    [1,F,W] in the resolution of `layer` over the model window.  Returns the updated (top, bottom).
    kv_cache_dtype: `sample_model`'s key/value cache format (None: the switch ISI_DECODE_KV).
    num_variations = N: N alternatives for the request, returned as (top [N,F_t,T], bottom [N,F_b,T_b]).  The prior of
    `layer` samples N variations over one shared source (`sample_model(num_variations=N)`); after a top-layer change the
    bottom prior has N different conditions and runs as an ordinary batch of N.
    return_scores: the result is (top, bottom, log_likelihood) -- log_likelihood float32 [N] ([1] without num_variations):
    the sum of the sampled tokens' model log-probabilities (`sample_model(return_log_probs=True)`) over the stages that ran,
    top then bottom.  sort_by_likelihood (needs return_scores): the variations in descending order of that score, ties in
    their original order.  Uniform sampling draws from no model distribution: it has no score (ValueError).
    allowed_codes_top / allowed_codes_bottom, code_bias_top / code_bias_bottom (with code_bias_map_top / code_bias_map_bottom
    over the window): `sample_model`'s options for the stage of that layer -- e.g. allowed_codes_top =
    `sample.codes_in_use(other_top, n)` regenerates the region from another sound's palette."""
    _check_score_options(return_scores, sort_by_likelihood, uniform_sampling)
    sampling_kwargs, bias = _split_code_bias(sampling_kwargs, uniform_sampling)
    if num_variations is not None:
        sampling_kwargs = dict(sampling_kwargs, _code_bias=bias)
        return _timerange_change_variations(transformer_top, transformer_bottom, top_code, bottom_code, mask, layer,
                                            start_index_top, temperature, class_conditioning_top,
                                            class_conditioning_bottom, device, uniform_sampling, generator, kv_cache_dtype,
                                            int(num_variations), sampling_kwargs, return_scores, sort_by_likelihood)
    (s_top, e_top), (s_bot, e_bot), ratio_t = _windows(top_code, bottom_code, transformer_top, transformer_bottom,
                                                        start_index_top)
    top_frame = top_code[..., s_top:e_top]
    bottom_frame = bottom_code[..., s_bot:e_bot]
    mask = mask.to(device)
    ti_top = make_time_indexes(s_top, top_code.shape[-1], transformer_top.shape[-1])
    ti_bottom = make_time_indexes(s_bot, bottom_code.shape[-1], transformer_bottom.shape[-1])
    common = dict(device=device, batch_size=1, temperature=temperature, generator=generator,
                  kv_cache_dtype=kv_cache_dtype, **sampling_kwargs)
    scores = []                        # per stage: [1] float64 sums of the sampled tokens' log-probabilities

    def resample(model, condition, initial, m, cls, ti_src, ti_tgt, steer):
        if uniform_sampling:
            rnd = torch.randint(0, model.n_class_target, initial.shape, generator=generator).to(initial.device)
            return torch.where(m, rnd, initial)
        out = sample_model(model=model, condition=condition, codemap_size=model.shape, class_conditioning=cls,
                           initial_code=initial, mask=m, time_indexes_source=ti_src, time_indexes_target=ti_tgt,
                           return_log_probs=return_scores, **steer, **common)
        if return_scores:
            scores.append(_stage_score(out[1]))
            return out[0]
        return out

    top_code, bottom_code = top_code.clone(), bottom_code.clone()
    if layer == 'bottom':
        bottom_code[..., s_bot:e_bot] = resample(transformer_bottom, top_frame, bottom_frame, mask,
                                                 class_conditioning_bottom, ti_top, ti_bottom, bias['bottom'])
    elif layer == 'top':
        condition = top_frame if transformer_top.self_conditional_model else None
        new_top = resample(transformer_top, condition, top_frame, mask, class_conditioning_top, ti_top, ti_top, bias['top'])
        top_code[..., s_top:e_top] = new_top
        ratio_f = transformer_bottom.shape[0] // transformer_top.shape[0]
        mask_bottom = mask.repeat_interleave(ratio_f, -2).repeat_interleave(ratio_t, -1)
        bottom_code[..., s_bot:e_bot] = resample(transformer_bottom, new_top, bottom_frame, mask_bottom,
                                                 class_conditioning_bottom, ti_top, ti_bottom, bias['bottom'])
    else:
        raise ValueError(f"unknown layer {layer}")
    if return_scores:
        return _ranked(top_code, bottom_code, scores, sort_by_likelihood)
    return top_code, bottom_code


# what `timerange_change` accepts by keyword beyond its positional arguments: its own options and, through **sampling_kwargs,
# those of `sample_model` that it does not set itself
_TIMERANGE_CHANGE_KEYWORDS = frozenset(
    {name for name, par in inspect.signature(timerange_change).parameters.items()
     if par.kind is par.POSITIONAL_OR_KEYWORD and par.default is not par.empty}
    | set(inspect.signature(sample_model).parameters)
    - {'model', 'device', 'batch_size', 'temperature', 'condition', 'codemap_size', 'class_conditioning', 'initial_code',
       'mask', 'time_indexes_source', 'time_indexes_target', 'return_log_probs', 'num_variations', 'generator',
       'kv_cache_dtype'})


@torch.no_grad()
def uncertainty(transformer_top, transformer_bottom, top_code: torch.Tensor, bottom_code: torch.Tensor,
                mask: Optional[torch.Tensor], layer: str, start_index_top: int,
                class_conditioning_top: Mapping[str, torch.Tensor], class_conditioning_bottom: Mapping[str, torch.Tensor],
                device, top_n: int = 0):
    """`sample.codemap_statistics` of the prior of `layer` over the model window starting at `start_index_top` -- the
    window, the source and the time indexes `timerange_change` would sample with: the top prior reads the top window
    through its encoder (mask tokens under `mask`), the bottom prior the top window as its condition.  top_code [1, F_t, T],
    bottom_code [1, F_b, T_b], mask bool [1, F, W] in the resolution of `layer` (None: every position, and see
    `codemap_statistics` on a self-conditional prior without a mask).  Returns its maps over the window: log_probs, entropy,
    rank [1, F, W], top_codes, top_log_probs [1, F, W, top_n]."""
    (s_top, e_top), (s_bot, e_bot), _ = _windows(top_code, bottom_code, transformer_top, transformer_bottom, start_index_top)
    top_frame = top_code[..., s_top:e_top]
    ti_top = make_time_indexes(s_top, top_code.shape[-1], transformer_top.shape[-1])
    if layer == 'top':
        condition = top_frame if transformer_top.self_conditional_model else None
        return codemap_statistics(transformer_top, device, top_frame, condition=condition,
                                  class_conditioning=class_conditioning_top, mask=mask, time_indexes_source=ti_top,
                                  time_indexes_target=ti_top, top_n=top_n)
    if layer == 'bottom':
        ti_bottom = make_time_indexes(s_bot, bottom_code.shape[-1], transformer_bottom.shape[-1])
        return codemap_statistics(transformer_bottom, device, bottom_code[..., s_bot:e_bot], condition=top_frame,
                                  class_conditioning=class_conditioning_bottom, mask=mask, time_indexes_source=ti_top,
                                  time_indexes_target=ti_bottom, top_n=top_n)
    raise ValueError(f"unknown layer {layer}")


def select_unlikely(log_probs: torch.Tensor, region: torch.Tensor, fraction: Optional[float] = None,
                    log_prob_below: Optional[float] = None) -> torch.Tensor:
    """The tokens of `region` (bool, the shape of `log_probs`) to sample again -- a bool mask of that shape, a subset of the
    region.  Exactly one rule (else ValueError): fraction in [0, 1] -- the ceil(fraction * |region|) tokens of lowest
    log-probability, equal values in the order of the flattened tensors (`resample_unlikely` passes sequences: ties go in
    the order the prior decodes them); log_prob_below -- every token whose log-probability lies below the threshold.
    Values outside the region are never looked at.  A pure function of its tensors."""
    if (fraction is None) == (log_prob_below is None):
        raise ValueError("select_unlikely: give exactly one of fraction and log_prob_below")
    if tuple(region.shape) != tuple(log_probs.shape) or region.dtype != torch.bool:
        raise ValueError(f"select_unlikely: region {region.dtype} {tuple(region.shape)} for log_probs {tuple(log_probs.shape)}")
    region = region.to(log_probs.device)
    if log_prob_below is not None:
        return region & (log_probs < log_prob_below)
    if not 0.0 <= fraction <= 1.0:
        raise ValueError(f"select_unlikely: fraction must lie in [0, 1], not {fraction}")
    inside = region.reshape(-1).nonzero()[:, 0]
    count = math.ceil(fraction * inside.numel())
    order = torch.argsort(log_probs.reshape(-1)[inside], stable=True)[:count]
    selected = torch.zeros(region.numel(), dtype=torch.bool, device=region.device)
    selected[inside[order]] = True
    return selected.reshape(region.shape)


@torch.no_grad()
def resample_unlikely(transformer_top, transformer_bottom, top_code: torch.Tensor, bottom_code: torch.Tensor,
                      mask: torch.Tensor, layer: str, start_index_top: int, temperature: float,
                      class_conditioning_top: Mapping[str, torch.Tensor],
                      class_conditioning_bottom: Mapping[str, torch.Tensor], device, fraction: Optional[float] = None,
                      log_prob_below: Optional[float] = None, **timerange_change_kwargs) -> Tuple[torch.Tensor, ...]:
    """"Fix what sounds wrong, keep the rest": `mask` (bool [1, F, W] in the resolution of `layer`) is the region the caller
    allows to change; the window is scored under it (`uncertainty`), `select_unlikely` picks the tokens inside it --
    `fraction`: that share of the region, least likely first; `log_prob_below`: every token below the threshold; exactly
    one of the two -- and `timerange_change` samples the selection again: after a top change the bottom prior runs under
    the up-sampled selection, as always.  Everything else (generator, kv_cache_dtype, num_variations, return_scores,
    sort_by_likelihood, top_k_sampling_k, top_p_sampling_p, ...) goes to `timerange_change` unchanged.  Returns its result
    with the selected mask appended: (top, bottom[, log_likelihood], selected).  An empty selection samples nothing and
    returns the inputs -- with num_variations = N as N equal rows, with return_scores a log-likelihood of 0."""
    if (fraction is None) == (log_prob_below is None):
        raise ValueError("resample_unlikely: give exactly one of fraction and log_prob_below")
    kw = timerange_change_kwargs
    _check_score_options(kw.get('return_scores'), kw.get('sort_by_likelihood'), kw.get('uniform_sampling'))
    unknown = set(kw) - _TIMERANGE_CHANGE_KEYWORDS - _CODE_BIAS_KEYWORDS      # (checked here: an empty selection never reaches timerange_change)
    if unknown:
        raise TypeError(f"resample_unlikely: unexpected keyword argument(s) {sorted(unknown)}")
    stats = uncertainty(transformer_top, transformer_bottom, top_code, bottom_code, mask, layer, start_index_top,
                        class_conditioning_top, class_conditioning_bottom, device)
    helper = (transformer_top if layer == 'top' else transformer_bottom).target_codemaps_helper
    selected = helper.to_time_frequency_map(select_unlikely(
        helper.to_sequence(stats.log_probs), helper.to_sequence(mask.to(stats.log_probs.device)), fraction, log_prob_below))
    if not bool(selected.any()):
        N = kw.get('num_variations')
        rows = 1 if N is None else int(N)
        if rows < 1:
            raise ValueError(f"num_variations must be at least 1, not {N}")
        out = (top_code.clone(), bottom_code.clone()) if N is None else (top_code.repeat(rows, 1, 1), bottom_code.repeat(rows, 1, 1))
        if kw.get('return_scores'):
            out += (torch.zeros(rows, dtype=torch.float32, device=stats.log_probs.device),)
        return out + (selected,)
    return timerange_change(transformer_top, transformer_bottom, top_code, bottom_code, selected, layer, start_index_top,
                            temperature, class_conditioning_top, class_conditioning_bottom, device, **kw) + (selected,)


def _stage_score(log_probs: torch.Tensor) -> torch.Tensor:
    """[B, F, T] token log-probabilities of one stage (0.0 where nothing was sampled) -> [B] sums, in float64."""
    return log_probs.double().sum(dim=(1, 2))


def _ranked(top, bottom, scores, sort_by_likelihood: bool):
    """(top, bottom, log_likelihood [N] float32): the stages' sums added in the order they ran; sorted on request by
    descending score (a stable sort: ties keep their original order)."""
    total = scores[0]
    for s in scores[1:]:
        total = total + s
    total = total.float()
    if sort_by_likelihood:
        order = torch.argsort(total, descending=True, stable=True)
        top, bottom, total = top[order.to(top.device)], bottom[order.to(bottom.device)], total[order]
    return top, bottom, total


def _timerange_change_variations(transformer_top, transformer_bottom, top_code, bottom_code, mask, layer, start_index_top,
                                 temperature, class_conditioning_top, class_conditioning_bottom, device, uniform_sampling,
                                 generator, kv_cache_dtype, N, sampling_kwargs, return_scores=False,
                                 sort_by_likelihood=False):
    if N < 1:
        raise ValueError(f"num_variations must be at least 1, not {N}")
    if layer not in ('top', 'bottom'):
        raise ValueError(f"unknown layer {layer}")
    (s_top, e_top), (s_bot, e_bot), ratio_t = _windows(top_code, bottom_code, transformer_top, transformer_bottom,
                                                        start_index_top)
    top_frame = top_code[..., s_top:e_top]
    bottom_frame = bottom_code[..., s_bot:e_bot]
    mask = mask.to(device)
    ti_top = make_time_indexes(s_top, top_code.shape[-1], transformer_top.shape[-1])
    ti_bottom = make_time_indexes(s_bot, bottom_code.shape[-1], transformer_bottom.shape[-1])
    sampling_kwargs = dict(sampling_kwargs)
    bias = sampling_kwargs.pop('_code_bias')           # timerange_change's per-layer options
    common = dict(device=device, temperature=temperature, generator=generator, kv_cache_dtype=kv_cache_dtype,
                  return_log_probs=return_scores, **sampling_kwargs)
    scores = []

    def scored(out):                   # a sample_model result: the codes; the stage's score is kept aside
        if return_scores:
            scores.append(_stage_score(out[1]))
            return out[0]
        return out

    def variations(model, condition, initial, m, cls, ti_src, ti_tgt, steer):      # N rows over one request
        if uniform_sampling:
            rnd = torch.randint(0, model.n_class_target, (N,) + tuple(initial.shape[1:]), generator=generator).to(initial.device)
            return torch.where(m, rnd, initial)
        return scored(sample_model(model=model, batch_size=1, num_variations=N, condition=condition, codemap_size=model.shape,
                                   class_conditioning=cls, initial_code=initial, mask=m, time_indexes_source=ti_src,
                                   time_indexes_target=ti_tgt, **steer, **common))

    top_out = top_code.repeat(N, 1, 1)
    bottom_out = bottom_code.repeat(N, 1, 1)
    if layer == 'bottom':
        bottom_out[..., s_bot:e_bot] = variations(transformer_bottom, top_frame, bottom_frame, mask,
                                                  class_conditioning_bottom, ti_top, ti_bottom, bias['bottom'])
        if return_scores:
            return _ranked(top_out, bottom_out, scores, sort_by_likelihood)
        return top_out, bottom_out
    condition = top_frame if transformer_top.self_conditional_model else None
    new_top = variations(transformer_top, condition, top_frame, mask, class_conditioning_top, ti_top, ti_top, bias['top'])
    top_out[..., s_top:e_top] = new_top
    ratio_f = transformer_bottom.shape[0] // transformer_top.shape[0]
    mask_bottom = mask.repeat_interleave(ratio_f, -2).repeat_interleave(ratio_t, -1)
    initial = bottom_frame.repeat(N, 1, 1)
    if uniform_sampling:
        rnd = torch.randint(0, transformer_bottom.n_class_target, initial.shape, generator=generator).to(initial.device)
        bottom_out[..., s_bot:e_bot] = torch.where(mask_bottom, rnd, initial)
    else:
        # N different conditions: an ordinary batch of N (one class value expands over the rows)
        bottom_out[..., s_bot:e_bot] = scored(sample_model(
            model=transformer_bottom, batch_size=N, condition=new_top, codemap_size=transformer_bottom.shape,
            class_conditioning=class_conditioning_bottom, initial_code=initial, mask=mask_bottom,
            time_indexes_source=ti_top, time_indexes_target=ti_bottom, **bias['bottom'], **common))
    if return_scores:
        return _ranked(top_out, bottom_out, scores, sort_by_likelihood)
    return top_out, bottom_out


def _cat_classes(dicts) -> Mapping[str, torch.Tensor]:
    return {k: torch.cat([torch.as_tensor(d[k]).long().reshape(-1) for d in dicts]) for k in dicts[0]}


@torch.no_grad()
def timerange_change_batch(transformer_top, transformer_bottom, requests: Sequence[Mapping], device,
                           kv_cache_dtype: Optional[torch.dtype] = None,
                           return_scores: bool = False) -> List[Tuple[torch.Tensor, ...]]:
    """Independent `timerange_change` requests in at most two ragged `sample_model` calls: every `layer='top'` request
    through the top prior together, then every request through the bottom prior together (a top request with the mask
    up-sampled over its new top map).  A request is a mapping with the arguments of `timerange_change` -- top_code,
    bottom_code, mask, layer, start_index_top, temperature, class_conditioning_top, class_conditioning_bottom and
    optionally top_k_sampling_k, top_p_sampling_p, uniform_sampling, allowed_codes_top / allowed_codes_bottom, code_bias_top /
    code_bias_bottom, code_bias_map_top / code_bias_map_bottom (the requests' distinct tables are stacked into one and a
    per-row map selects each request's rows; a request without them draws unbiased) -- and its own `generator`, from which its uniforms
    are drawn in the order `timerange_change` draws them (top stage, then bottom): result r equals `timerange_change` of
    request r alone with an equally seeded generator.  Returns one (top, bottom) pair per request; with return_scores one
    (top, bottom, log_likelihood [1]) triple, `timerange_change(return_scores=True)`'s (a request with uniform_sampling
    has no score: ValueError)."""
    ratio_f = transformer_bottom.shape[0] // transformer_top.shape[0]
    jobs = []
    for r in requests:
        if r['layer'] not in ('top', 'bottom'):
            raise ValueError(f"unknown layer {r['layer']}")
        if return_scores and r.get('uniform_sampling', False):
            raise ValueError("return_scores: uniform_sampling draws from no model distribution, there is no likelihood to report")
        (s_top, e_top), (s_bot, e_bot), ratio_t = _windows(r['top_code'], r['bottom_code'], transformer_top,
                                                            transformer_bottom, r['start_index_top'])
        _, steer = _split_code_bias(r, r.get('uniform_sampling', False))
        steer = {'top': _code_bias_rows(transformer_top, 1, **{n: steer['top'].get(n) for n in _CODE_BIAS_OPTIONS}),
                 'bottom': _code_bias_rows(transformer_bottom, 1, **{n: steer['bottom'].get(n) for n in _CODE_BIAS_OPTIONS})}
        jobs.append(dict(req=r, steer=steer, top=r['top_code'].clone(), bottom=r['bottom_code'].clone(), s_top=s_top, e_top=e_top,
                         s_bot=s_bot, e_bot=e_bot, ratio_t=ratio_t, mask=r['mask'].to(device), g=r.get('generator'),
                         ti_top=make_time_indexes(s_top, r['top_code'].shape[-1], transformer_top.shape[-1]),
                         ti_bottom=make_time_indexes(s_bot, r['bottom_code'].shape[-1], transformer_bottom.shape[-1])))

    def stacked_bias(model, batch, layer):      # one table of the batch's distinct tables, one map row per request
        tables, offsets, maps, n_rows = [], [], [], 0
        for j in batch:
            table, m = j['steer'][layer]
            if table is None:
                maps.append(torch.full((1,) + tuple(model.shape), -1, dtype=torch.int64))
                continue
            same = [k for k, t in enumerate(tables) if t.shape == table.shape and torch.equal(t, table)]
            if same:
                off = offsets[same[0]]
            else:
                off = n_rows
                tables.append(table)
                offsets.append(off)
                n_rows += table.shape[0]
            m = torch.zeros((1,) + tuple(model.shape), dtype=torch.int64) if m is None else m
            maps.append(torch.where(m >= 0, m + off, m))
        if not tables:
            return {}
        return dict(code_bias=torch.cat(tables), code_bias_map=torch.cat(maps))

    def run(model, batch, condition, initial, masks, cls_key, ti_src, ti_tgt, uniforms):
        req = [j['req'] for j in batch]
        return sample_model(
            **stacked_bias(model, batch, 'top' if cls_key == 'class_conditioning_top' else 'bottom'),
            model=model, device=device, batch_size=len(batch), codemap_size=model.shape,
            temperature=[float(q['temperature']) for q in req],
            condition=torch.cat(condition) if condition is not None else None,
            class_conditioning=_cat_classes([q[cls_key] for q in req]), initial_code=torch.cat(initial).to(device),
            mask=torch.cat(masks).to(device), time_indexes_source=torch.tensor(ti_src),
            time_indexes_target=torch.tensor(ti_tgt),
            top_k_sampling_k=[int(q.get('top_k_sampling_k', 0)) for q in req],
            top_p_sampling_p=[float(q.get('top_p_sampling_p', 0.0)) for q in req],
            uniforms=torch.cat(uniforms, 1), kv_cache_dtype=kv_cache_dtype, return_log_probs=return_scores)

    def scored(out, batch):            # a sample_model result: the codes; every row's stage score goes to its job
        if not return_scores:
            return out
        for k, j in enumerate(batch):
            j.setdefault('scores', []).append(_stage_score(out[1][k:k + 1]))
        return out[0]

    def draw(model, j, frame):        # timerange_change's draws from the request's generator, in its order
        if j['req'].get('uniform_sampling', False):
            return torch.randint(0, model.n_class_target, frame.shape, generator=j['g'])
        return torch.rand(model.target_transformer_sequence_length, 1, generator=j['g'])

    # stage 1: the top prior, every layer='top' request in one ragged call
    tops = [j for j in jobs if j['req']['layer'] == 'top']
    for j in tops:
        frame = j['top'][..., j['s_top']:j['e_top']]
        d = draw(transformer_top, j, frame)
        if j['req'].get('uniform_sampling', False):
            j['top'][..., j['s_top']:j['e_top']] = torch.where(j['mask'], d.to(frame.device), frame)
        else:
            j['u_top'] = d
    sampled = [j for j in tops if 'u_top' in j]
    if sampled:
        frames = [j['top'][..., j['s_top']:j['e_top']] for j in sampled]
        new_top = scored(run(transformer_top, sampled, frames if transformer_top.self_conditional_model else None, frames,
                             [j['mask'] for j in sampled], 'class_conditioning_top', [j['ti_top'] for j in sampled],
                             [j['ti_top'] for j in sampled], [j['u_top'] for j in sampled]), sampled)
        for k, j in enumerate(sampled):
            j['top'][..., j['s_top']:j['e_top']] = new_top[k:k + 1].to(j['top'].device)
    # stage 2: the bottom prior, every request in one ragged call
    for j in jobs:
        if j['req']['layer'] == 'top':
            j['mask'] = j['mask'].repeat_interleave(ratio_f, -2).repeat_interleave(j['ratio_t'], -1)
        frame = j['bottom'][..., j['s_bot']:j['e_bot']]
        d = draw(transformer_bottom, j, frame)
        if j['req'].get('uniform_sampling', False):
            j['bottom'][..., j['s_bot']:j['e_bot']] = torch.where(j['mask'], d.to(frame.device), frame)
        else:
            j['u_bot'] = d
    sampled = [j for j in jobs if 'u_bot' in j]
    if sampled:
        new_bottom = scored(run(transformer_bottom, sampled, [j['top'][..., j['s_top']:j['e_top']] for j in sampled],
                                [j['bottom'][..., j['s_bot']:j['e_bot']] for j in sampled], [j['mask'] for j in sampled],
                                'class_conditioning_bottom', [j['ti_top'] for j in sampled],
                                [j['ti_bottom'] for j in sampled], [j['u_bot'] for j in sampled]), sampled)
        for k, j in enumerate(sampled):
            j['bottom'][..., j['s_bot']:j['e_bot']] = new_bottom[k:k + 1].to(j['bottom'].device)
    if return_scores:
        return [_ranked(j['top'], j['bottom'], j['scores'], False) for j in jobs]
    return [(j['top'], j['bottom']) for j in jobs]


@torch.no_grad()
def generate(transformer_top, transformer_bottom, temperature: float,
             class_conditioning_top: Mapping[str, torch.Tensor],
             class_conditioning_bottom: Mapping[str, torch.Tensor], device,
             generator: Optional[torch.Generator] = None, kv_cache_dtype: Optional[torch.dtype] = None,
             **sampling_kwargs):
    sampling_kwargs = dict(sampling_kwargs, kv_cache_dtype=kv_cache_dtype)
    top = sample_model(model=transformer_top, device=device, batch_size=1, codemap_size=transformer_top.shape,
                       temperature=temperature, class_conditioning=class_conditioning_top, generator=generator,
                       **sampling_kwargs)
    bottom = sample_model(model=transformer_bottom, device=device, condition=top, batch_size=1,
                          codemap_size=transformer_bottom.shape, temperature=temperature,
                          class_conditioning=class_conditioning_bottom, generator=generator, **sampling_kwargs)
    return top, bottom


@torch.no_grad()
def erase(vqvae, top_code: torch.Tensor, bottom_code: torch.Tensor, mask: torch.Tensor, amplitude: float,
          start_index_top: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Subtract 200 * amplitude from the decoded log-magnitude under the (up-sampled, placed) mask and
    re-encode; mask bool [F_t, W] in top resolution."""
    spec = vqvae.decode_code(top_code, bottom_code)[0]
    logmag, IF = spec[0], spec[1]
    top = top_code[0]
    up_f, up_t = logmag.shape[0] // top.shape[0], logmag.shape[1] // top.shape[1]
    up = mask.to(logmag.device).float().flip(0).repeat_interleave(up_f, 0).repeat_interleave(up_t, 1).flip(0)
    amp = 200.0 * amplitude * up
    before = torch.zeros(logmag.shape[0], up_t * start_index_top, device=logmag.device)
    after = torch.zeros(logmag.shape[0], max(0, up_t * (top.shape[1] - (start_index_top + mask.shape[1]))),
                        device=logmag.device)
    amp = torch.cat([before, amp, after], 1)
    x = torch.stack([logmag - amp, IF], 0).unsqueeze(0).contiguous()
    _, _, _, new_top, new_bottom, *_ = vqvae.encode(x)
    return new_top, new_bottom


@torch.no_grad()
def codes_to_audio(vqvae, spectrograms_helper, top_code: torch.Tensor, bottom_code: torch.Tensor) -> torch.Tensor:
    return spectrograms_helper.to_audio(vqvae.decode_code(top_code, bottom_code))


def changed_cells(top0: torch.Tensor, bottom0: torch.Tensor, top1: torch.Tensor, bottom1: torch.Tensor) -> torch.Tensor:
    """Which cells of the top codemap an edit touched: bool [F_top, T_top] ([B, F_top, T_top] for batches of more than one
    sound), true where the top code differs or any bottom cell under it does.  Codemaps [F, T] or [B, F, T]."""
    maps = [torch.as_tensor(c).cpu() for c in (top0, bottom0, top1, bottom1)]
    maps = [c.unsqueeze(0) if c.dim() == 2 else c for c in maps]
    t0, b0, t1, b1 = maps
    if t0.shape != t1.shape or b0.shape != b1.shape or t0.dim() != 3 or b0.dim() != 3 or t0.shape[0] != b0.shape[0]:
        raise ValueError("changed_cells: the two sounds' codemaps must have equal shapes")
    (B, Ft, Tt), (_, Fb, Tb) = t0.shape, b0.shape
    if Fb % Ft or Tb % Tt:
        raise ValueError(f"changed_cells: bottom map {Fb} x {Tb} is no multiple of top map {Ft} x {Tt}")
    under = (b0 != b1).reshape(B, Ft, Fb // Ft, Tt, Tb // Tt).any(4).any(2)
    changed = (t0 != t1) | under
    return changed[0] if B == 1 else changed


def splice_weights(spectrograms_helper, mask_top: torch.Tensor, n_frames: int, feather_frames: int, halo_top: int = 1) -> torch.Tensor:
    """The weights `SpectrogramsHelper.to_audio_spliced` takes, from a mask over the top codemap: float32
    [1 or B, n_frames, n_fft / 2] on the CPU, 0 where the original is kept, above 0 where the sound is regenerated.

    mask_top bool [F_top, T_top] (or [B, F_top, T_top]; `changed_cells` makes one).  The mask is grown by `halo_top` cells
    in both directions (the decoder's receptive field changes the neighbours of a changed code too), repeated to
    spectrogram rows and frames (mask row i covers spectrogram rows [i up, (i + 1) up), lowest frequency first: the order
    of `erase` and, bottom-up, of `spectrogram_png`), and given linear ramps of `feather_frames` frames in time on both
    sides (1 - d / (feather_frames + 1) at distance d).  For a mel helper the rows are mel bands: a linear bin gets the
    mean of the bands it feeds, weighted with `_mel_matrix`; a bin that feeds none keeps the original.  Host, float64."""
    m = torch.as_tensor(mask_top).cpu()
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if m.dim() != 3:
        raise ValueError("splice_weights: mask_top must be [F_top, T_top] or [B, F_top, T_top]")
    _, Ft, Tt = m.shape
    rows, feather, halo = int(spectrograms_helper.n_bins), int(feather_frames), int(halo_top)
    if feather < 0 or halo < 0 or n_frames < 1 or n_frames % Tt or rows % Ft:
        raise ValueError(f"splice_weights: {n_frames} frames x {rows} rows is no multiple of the mask's {Tt} x {Ft}, "
                         "or a negative feather / halo")
    w = (m != 0).to(torch.float64)
    if halo:
        w = torch.nn.functional.max_pool2d(w.unsqueeze(1), 2 * halo + 1, stride=1, padding=halo).squeeze(1)
    w = w.repeat_interleave(rows // Ft, 1).repeat_interleave(n_frames // Tt, 2)          # [B, rows, frames]
    hard, w = w, w.clone()
    for d in range(1, min(feather, n_frames - 1) + 1):
        level = 1.0 - d / (feather + 1.0)
        w[..., d:] = torch.maximum(w[..., d:], level * hard[..., :-d])
        w[..., :-d] = torch.maximum(w[..., :-d], level * hard[..., d:])
    w = w.transpose(1, 2)                                                               # [B, frames, rows]
    if getattr(spectrograms_helper, 'mel', False):
        M = spectrograms_helper._mel_matrix().to(torch.float64)                          # [linear, mel]
        fed = M.sum(1)
        w = (w @ M.t()) / torch.where(fed > 0, fed, torch.ones_like(fed))
    return w.clamp(0.0, 1.0).to(torch.float32).contiguous()


@torch.no_grad()
def codes_to_audio_spliced(vqvae, spectrograms_helper, original_audio: torch.Tensor, top_code: torch.Tensor,
                           bottom_code: torch.Tensor, mask_top: Optional[torch.Tensor] = None,
                           feather_frames: Optional[int] = None, halo_top: int = 1) -> torch.Tensor:
    """`codes_to_audio` for an uploaded sound whose codes were edited: the upload's own samples wherever the edit does
    not reach, the decoded codes inside it, phase-locked to the upload at both seams (`to_audio_spliced`).

    original_audio: mono [samples] (or [B, samples]) at the models' rate, trimmed / zero-padded to the codes' duration as
    `analyze_audio` does.  mask_top bool [F_top, T_top]: the edited cells of the top map; None: the upload is encoded
    again and the cells whose codes differ are taken (`changed_cells`).  The mask is grown by `halo_top` cells and
    feathered over `feather_frames` frames (default: one top column's) -- `splice_weights`.  Unchanged codes return the
    upload itself.  Returns [B, samples]."""
    spec = vqvae.decode_code(top_code, bottom_code)
    B, n_frames = spec.shape[0], spec.shape[-1]
    duration_n = n_frames * spectrograms_helper.hop_length
    x = original_audio.to(device=spec.device, dtype=torch.float32).reshape(B, -1)[:, :duration_n]
    if x.shape[1] < duration_n:
        x = torch.nn.functional.pad(x, (0, duration_n - x.shape[1]))
    x = x.contiguous()
    if mask_top is None:
        _, _, _, top0, bottom0, *_ = vqvae.encode(spectrograms_helper.to_spectrogram(x))
        mask_top = changed_cells(top0, bottom0, top_code, bottom_code)
    if feather_frames is None:
        feather_frames = n_frames // top_code.shape[-1]
    weights = splice_weights(spectrograms_helper, mask_top, n_frames, feather_frames, halo_top)
    return spectrograms_helper.to_audio_spliced(spec, x, weights.to(spec.device))


def _sound_device(audio, vqvae, spectrograms_helper) -> torch.device:
    """where a sound is worked on: its own GPU, else the helper's device, else the model's"""
    if audio.is_cuda:
        return audio.device
    if getattr(spectrograms_helper, 'device', None) is not None:
        return spectrograms_helper.device
    return next(vqvae.parameters()).device if vqvae is not None else audio.device


@torch.no_grad()
def stretch_sound(vqvae, spectrograms_helper, audio: Optional[torch.Tensor] = None, codes=None, factor: float = 1.0,
                  keep_attack_s: float = 0.0, keep_release_s: float = 0.0) -> torch.Tensor:
    """A sound `factor` times as long at its own pitch; the first `keep_attack_s` and the last `keep_release_s` seconds keep
    their own rate ("hold this note longer but keep its attack").  Either `audio`, mono [samples] or [B, samples] at the
    models' rate (`GANsynth_pytorch.stretch.time_stretch` of its own STFT), or `codes` = (top_code, bottom_code), decoded at
    the other length (`SpectrogramsHelper.to_audio_stretched`: no second analysis).  Returns audio [.., samples].
    ValueError for a factor that is not positive and finite or kept seconds that do not fit."""
    from GANsynth_pytorch import stretch
    if (audio is None) == (codes is None):
        raise ValueError("stretch_sound: give exactly one of audio and codes")
    if audio is not None:
        x = audio.to(device=_sound_device(audio, vqvae, spectrograms_helper), dtype=torch.float32)
        return stretch.time_stretch(spectrograms_helper, x, factor, keep_attack_s, keep_release_s)
    top_code, bottom_code = codes
    spec = vqvae.decode_code(top_code, bottom_code)
    head = stretch._seconds_to_frames(spectrograms_helper, keep_attack_s, "keep_attack_s")
    tail = stretch._seconds_to_frames(spectrograms_helper, keep_release_s, "keep_release_s")
    positions = stretch.stretch_positions(spec.shape[-1], factor=factor, keep_head=head, keep_tail=tail)
    return spectrograms_helper.to_audio_stretched(spec, positions.to(spec.device))


@torch.no_grad()
def transpose_sound(vqvae, spectrograms_helper, audio: torch.Tensor, semitones: Optional[float] = None,
                    to_pitch: Optional[float] = None, like: Optional[torch.Tensor] = None, re_encode: bool = True,
                    preserve_formants: bool = False):
    """A sound at another pitch and its own length: (audio, top_code, bottom_code).  Exactly one of `semitones` (may be
    fractional), `to_pitch` (a MIDI number) and `like` (another sound, whose estimated pitch is the target).  The last two
    take the source's pitch from `GANsynth_pytorch.pitch.estimate_pitch`, unrounded; ValueError when a sound they need the
    pitch of is unvoiced.  Mono audio [samples] at the models' rate.  The codes come from `analyze_audio` of the result
    (None, None with re_encode=False), so that it can be morphed, searched and inpainted like any other sound.
    preserve_formants: the resonances stay where they were (`GANsynth_pytorch.stretch.transpose`); the envelope's order comes
    from the source's pitch, the estimate made here where `to_pitch` or `like` needed one."""
    from GANsynth_pytorch import stretch
    from GANsynth_pytorch.pitch import estimate_pitch as estimate
    if sum(v is not None for v in (semitones, to_pitch, like)) != 1:
        raise ValueError("transpose_sound: give exactly one of semitones, to_pitch and like")
    device = _sound_device(audio, vqvae, spectrograms_helper)
    x = audio.to(device=device, dtype=torch.float32).reshape(-1)

    def pitch_of(sound, name):
        midi = float(estimate(sound, int(spectrograms_helper.fs_hz))[0])
        if midi != midi:
            raise ValueError(f"transpose_sound: {name} is unvoiced, it has no pitch to transpose from or to")
        return midi

    if semitones is None:
        target = float(to_pitch) if to_pitch is not None else \
            pitch_of(like.to(device=device, dtype=torch.float32).reshape(-1), "the sound to be like")
        if not math.isfinite(target):
            raise ValueError(f"transpose_sound: to_pitch must be finite, got {target}")
        own = pitch_of(x, "the sound")
        semitones = target - own
    else:
        own = None
    if preserve_formants:
        y = stretch.transpose(spectrograms_helper, x, float(semitones), preserve_formants=True, pitch=own)
    else:
        y = stretch.transpose(spectrograms_helper, x, float(semitones))
    if not re_encode:
        return y, None, None
    top_code, bottom_code = analyze_audio(vqvae, spectrograms_helper, y, y.numel(), device)
    return y, top_code, bottom_code


@torch.no_grad()
def shift_formants_sound(vqvae, spectrograms_helper, audio: torch.Tensor, semitones: float, re_encode: bool = True):
    """A sound at its own pitch and length with its formants `semitones` higher (lower when negative): (audio, top_code,
    bottom_code), like `transpose_sound` (`GANsynth_pytorch.stretch.shift_formants`: a darker or brighter instrument playing
    the same note).  ValueError for a value that is not finite.  Mono audio [samples] at the models' rate."""
    from GANsynth_pytorch import stretch
    device = _sound_device(audio, vqvae, spectrograms_helper)
    x = audio.to(device=device, dtype=torch.float32).reshape(-1)
    y = stretch.shift_formants(spectrograms_helper, x, semitones)
    if not re_encode:
        return y, None, None
    top_code, bottom_code = analyze_audio(vqvae, spectrograms_helper, y, y.numel(), device)
    return y, top_code, bottom_code


def contour_curve(track, clip_pitch: float, n_samples: int, fs_hz: int, max_correction: float = 1.5) -> torch.Tensor:
    """A `PitchTrack` of one clip -> its pitch per sample, float64 [n_samples] on the host, in MIDI numbers: linear between
    the frame times, held outside.  Frames that are unvoiced, or further than `max_correction` semitones from the clip's
    pitch (an octave error would otherwise become a 12-semitone jump), take the nearest accepted frame's value.
    ValueError when no frame is accepted."""
    import numpy as np
    midi = track.midi.reshape(-1).double().cpu().numpy()
    ok = track.voiced.reshape(-1).cpu().numpy() & (np.abs(midi - clip_pitch) <= float(max_correction))
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        raise ValueError("no frame of the sound has a pitch near the clip's: nothing to follow")
    nearest = idx[np.abs(np.arange(midi.size)[:, None] - idx[None, :]).argmin(1)]
    times = track.times_s.double().cpu().numpy()
    return torch.from_numpy(np.interp(np.arange(int(n_samples)) / float(fs_hz), times, midi[nearest]))


@torch.no_grad()
def bend_sound(vqvae, spectrograms_helper, audio: torch.Tensor, curve=None, vibrato=None, glide=None, flatten: bool = False,
               to_pitch: Optional[float] = None, contour_of: Optional[torch.Tensor] = None, times_s=None,
               max_correction: float = 1.5, re_encode: bool = True, preserve_formants: bool = False):
    """A sound with its pitch contour redrawn, at its own length: (audio, top_code, bottom_code), like `transpose_sound`.
    Exactly one of
      curve       semitones over time: control points at `times_s` (seconds; linear between, held outside), or one value per sample
      vibrato     (rate_hz, depth_cents): added from the start, faded in over 0.1 s
      glide       (from_semitones, to_semitones) over the whole sound
      flatten     bend by target - contour(t): the sound's own vibrato and drift removed.  The target is `to_pitch` (a MIDI
                  number: "tune this upload to the class the prior is told"), else the clip's own pitch rounded
      contour_of  another sound, whose deviation from its own median pitch is added ("sing it like that one")
    The contours come from `GANsynth_pytorch.pitch.pitch_contour` (`contour_curve`: frames that are unvoiced or further than
    `max_correction` semitones from their clip's pitch take the nearest accepted frame's value).  ValueError for an unvoiced
    sound where a contour is needed and for curves `GANsynth_pytorch.bend.curve` refuses.  Mono audio [samples] at the
    models' rate; the codes come from `analyze_audio` of the result (None, None with re_encode=False).
    preserve_formants: the resonances stay where they were (`GANsynth_pytorch.bend.bend`); the envelope's order comes from
    the clip's pitch, the estimate made here where a contour needed one."""
    from GANsynth_pytorch import bend as _bend
    from GANsynth_pytorch.pitch import estimate_pitch as estimate, pitch_contour
    chosen = sum([curve is not None, vibrato is not None, glide is not None, bool(flatten), contour_of is not None])
    if chosen != 1:
        raise ValueError("bend_sound: give exactly one of curve, vibrato, glide, flatten and contour_of")
    if to_pitch is not None and not flatten:
        raise ValueError("bend_sound: to_pitch belongs to flatten")
    device = _sound_device(audio, vqvae, spectrograms_helper)
    x = audio.to(device=device, dtype=torch.float32).reshape(-1)
    fs_hz = int(spectrograms_helper.fs_hz)

    def contour(sound, name):
        midi = float(estimate(sound, fs_hz)[0])
        if midi != midi:
            raise ValueError(f"bend_sound: {name} is unvoiced, it has no pitch contour")
        return contour_curve(pitch_contour(sound, fs_hz), midi, x.numel(), fs_hz, max_correction), midi

    keep = dict(preserve_formants=True) if preserve_formants else {}
    if vibrato is not None:
        rate_hz, depth_cents = vibrato
        y = _bend.vibrato(spectrograms_helper, x, rate_hz, depth_cents, **keep)
    elif glide is not None:
        y = _bend.glide(spectrograms_helper, x, glide[0], glide[1], **keep)
    elif curve is not None:
        y = _bend.bend(spectrograms_helper, x, curve, times_s, **keep)
    elif flatten:
        own, clip = contour(x, "the sound")
        target = float(to_pitch) if to_pitch is not None else float(round(clip))
        if not math.isfinite(target):
            raise ValueError(f"bend_sound: to_pitch must be finite, got {target}")
        if preserve_formants:
            keep["pitch"] = clip
        y = _bend.bend(spectrograms_helper, x, target - own, **keep)
    else:
        other, _ = contour(contour_of.to(device=device, dtype=torch.float32).reshape(-1), "the sound whose contour is taken")
        y = _bend.bend(spectrograms_helper, x, other - other.median(), **keep)
    if not re_encode:
        return y, None, None
    top_code, bottom_code = analyze_audio(vqvae, spectrograms_helper, y, y.numel(), device)
    return y, top_code, bottom_code


@torch.no_grad()
def top_conditioned_sample(vqvae, transformer_bottom, spectrograms_helper, top_code: torch.Tensor, temperature: float,
                           class_conditioning_bottom, device, top_k_sampling_k: int = 0, top_p_sampling_p: float = 0.0,
                           generator=None, uniforms=None, kv_cache_dtype: Optional[torch.dtype] = None):
    """The compute of `/top-conditioned-sample` (flask_server.py:1049-1110): ONE top codemap, a batch of bottom codemaps
    drawn from the bottom prior -- one per entry of the per-row class conditioning (the route passes a pitch range:
    `make_conditioning_tensors({'pitch': (lo, hi), ...})`, sample.py:68-101) --, decoded and turned into audio.
    The batch goes through the native batched decoder in one call (rows of a stage as one launch / matrix tiles beyond 16
    sequences).  Returns (bottom_code [N, F_b, T_b], audio [N, samples])."""
    from sample import sample_model
    n = max(int(torch.as_tensor(v).numel()) for v in class_conditioning_bottom.values())
    top = top_code.to(device).expand(n, -1, -1)
    bottom = sample_model(transformer_bottom, device, n, transformer_bottom.shape, temperature, condition=top,
                          class_conditioning=class_conditioning_bottom, top_k_sampling_k=top_k_sampling_k,
                          top_p_sampling_p=top_p_sampling_p, generator=generator, uniforms=uniforms,
                          kv_cache_dtype=kv_cache_dtype)
    audio = spectrograms_helper.to_audio(vqvae.decode_code(top, bottom))
    return bottom, audio


def adapt_duration(duration_n: int, fs_hz: int, max_sound_duration_s: float, top_resolution_n: int, top_duration: int) -> int:
    """flask_server.py:602-621: trim to the maximal duration, round to the resolution of the VQ-VAE's top level, at least
    one transformer window."""
    duration_n = min(max_sound_duration_s * fs_hz, duration_n)
    return int(top_resolution_n * max(top_duration, round(duration_n / top_resolution_n)))


@torch.no_grad()
def top_resolution_n(vqvae, transformer_top, transformer_bottom, spectrograms_helper, device) -> int:
    """Samples of audio per column of the top codemap (flask_server.py:582-599): from a decoded dummy map."""
    dummy_top = torch.zeros((1,) + tuple(transformer_top.shape), dtype=torch.long, device=device)
    dummy_bottom = torch.zeros((1,) + tuple(transformer_bottom.shape), dtype=torch.long, device=device)
    audio = spectrograms_helper.to_audio(vqvae.decode_code(dummy_top, dummy_bottom))
    return audio.shape[-1] // transformer_top.shape[1]


@torch.no_grad()
def analyze_audio(vqvae, spectrograms_helper, audio: torch.Tensor, duration_n: int, device, fs_hz: Optional[int] = None):
    """The compute of `/analyze-audio` (flask_server.py:624-667): mono audio [samples] at the models' rate, trimmed /
    zero-padded to `duration_n` (what `from_wavfile(path, duration_n=...)` does), -> spectrogram -> `VQVAE.encode` ->
    (top_code, bottom_code).  `fs_hz`: the rate of `audio` when it is not the models' -- it is resampled first
    (GANsynth_pytorch/resample.py; `duration_n` counts samples at the models' rate)."""
    x = audio.to(device=device, dtype=torch.float32).reshape(-1)
    if fs_hz is not None and int(fs_hz) != int(spectrograms_helper.fs_hz):
        from GANsynth_pytorch.resample import resample
        x = resample(x, fs_hz, spectrograms_helper.fs_hz)
    x = x[:duration_n]
    if x.numel() < duration_n:
        x = torch.nn.functional.pad(x, (0, duration_n - x.numel()))
    spec = spectrograms_helper.to_spectrogram(x.unsqueeze(0))
    _, _, _, top_code, bottom_code, *_ = vqvae.encode(spec)
    return top_code, bottom_code


@torch.no_grad()
def estimate_pitch(audio: torch.Tensor, spectrograms_helper, fs_hz: Optional[int] = None, pitch_range=None):
    """The `pitch` conditioning of a sound whose pitch nobody knows (an upload): (MIDI number or None, confidence).
    Mono audio [samples] on the GPU at `fs_hz` (default: the models' rate); the estimate of
    `GANsynth_pytorch.pitch.estimate_pitch` rounded to the nearest MIDI number and clamped to `pitch_range`, the values
    the priors were trained with (callers pass the pitch label encoder's classes).  None when no frame is voiced
    (noise, silence); the confidence is the voiced share of the frames."""
    from GANsynth_pytorch.pitch import estimate_pitch as estimate
    rate = int(spectrograms_helper.fs_hz if fs_hz is None else fs_hz)
    midi, confidence = estimate(audio.to(torch.float32).reshape(-1), rate)
    midi, confidence = float(midi), float(confidence)
    if midi != midi:
        return None, confidence
    pitch = int(math.floor(midi + 0.5))
    if pitch_range is not None:
        values = [int(v) for v in pitch_range]
        pitch = min(max(pitch, min(values)), max(values))
    return pitch, confidence


def resize_codemaps_repeat_last(top_code: torch.Tensor, bottom_code: torch.Tensor, duration_top: int):
    """flask_server.py:314-330: cut to `duration_top` columns of the top map (and the matching number of the bottom map);
    a shorter map is continued with its last column."""
    ratio = bottom_code.shape[-1] // top_code.shape[-1]

    def resize(codemap, duration):
        codemap = codemap[..., :duration]
        if codemap.shape[-1] < duration:
            codemap = torch.cat([codemap, codemap[..., -1:].expand(*codemap.shape[:-1], duration - codemap.shape[-1])], -1)
        return codemap
    return resize(top_code, duration_top), resize(bottom_code, ratio * duration_top)


def _check_layer(layer: str) -> None:
    if layer not in ('top', 'bottom'):
        raise ValueError(f"unknown layer {layer}")


def _one_map(m: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A codemap or a mask [F, T] (or [1, F, T], [1, 1, F, T]) as [1, F, T]."""
    return None if m is None else m.reshape(1, *m.shape[-2:])


def _bottom_mask(mask: torch.Tensor, ratio_f: int, ratio_t: int) -> torch.Tensor:
    """A top-layer mask in the bottom layer's resolution, as `timerange_change` extends it."""
    return mask.repeat_interleave(ratio_f, -2).repeat_interleave(ratio_t, -1)


def _search_window(index, search, window, vectors: bool = False, **options):
    """The body of the `similar_*` functions: `window` -- what `_similar_window` or `_fragment_window` returns -- through
    `search`, one of the index's `search_*` methods, and its answer as the list they return: ((top, bottom), attributes,
    distance[, shift_top]) per item.  vectors: the maps are laid out [1, D, F, T] and go in as `*_vectors`."""
    top, bottom, mask_top, mask_bottom, two = window
    on_device = (lambda m: m.permute(0, 2, 3, 1).to(index.device)) if vectors else (lambda m: m.to(index.device))
    form = 'vectors' if vectors else 'code'
    indices, *shifts, distances = search(**{f'top_{form}': on_device(top), f'bottom_{form}': on_device(bottom) if two else None},
                                         mask_top=mask_top, mask_bottom=mask_bottom, **options)
    out = []
    for i, d, *shift in zip(indices.tolist(), distances.tolist(), *(s.tolist() for s in shifts)):
        item_top, item_bottom, _ = index[i]
        out.append(((item_top.unsqueeze(0), None if item_bottom is None else item_bottom.unsqueeze(0)),
                    index.decoded_attributes(i), d, *shift))
    return out


def _similar_window(index, top_code, bottom_code, mask, layer: str, start_index_top: int):
    """What `similar_sounds` compares, for maps whose last two dimensions are [F, T] (codes [1, F, T]; vectors laid out
    [1, D, F, T]): (top_frame, bottom_frame, mask_top, mask_bottom, two) -- the window of the stored duration from
    `start_index_top` on, a shorter map continued with its last column under a mask, the caller's mask merged in."""
    _check_layer(layer)
    two = bottom_code is not None and index.bottom_shape is not None
    shape_top = index.top_shape
    shape_bottom = index.bottom_shape if two else (shape_top[0], shape_top[1])
    bottom_ref = bottom_code if two else top_code
    window = _windows(top_code, bottom_ref, SimpleNamespace(shape=shape_top), SimpleNamespace(shape=shape_bottom),
                      start_index_top)
    (s_top, e_top), (s_bot, e_bot), ratio_t = window
    top_frame, bottom_frame = top_code[..., s_top:e_top], bottom_ref[..., s_bot:e_bot]
    if top_frame.shape[-1] < 1:
        raise ValueError(f"start_index_top {start_index_top} lies beyond the top map's {top_code.shape[-1]} columns")
    known_top = top_frame.shape[-1]                   # columns of the window the sound really has
    top_frame, bottom_frame = resize_codemaps_repeat_last(top_frame, bottom_frame, shape_top[1])
    device = index.device
    mask_top = torch.zeros((1,) + tuple(shape_top), dtype=torch.bool, device=device)
    mask_top[..., known_top:] = True
    mask_bottom = None
    if two:
        mask_bottom = torch.zeros((1,) + tuple(shape_bottom), dtype=torch.bool, device=device)
        mask_bottom[..., ratio_t * known_top:] = True
    if mask is not None:
        mask = mask.to(device).reshape(1, *mask.shape[-2:])
        rows = shape_top[0] if layer == 'top' else shape_bottom[0]
        if mask.dtype != torch.bool or mask.shape[-2] != rows:
            raise ValueError(f"mask: expected bool [1, {rows}, W] in the {layer} layer's resolution, got "
                             f"{mask.dtype} {tuple(mask.shape)}")
        if layer == 'top':
            mask_top[..., :mask.shape[-1]] |= mask[..., :shape_top[1]]
            if two:
                up = _bottom_mask(mask, shape_bottom[0] // shape_top[0], ratio_t)
                mask_bottom[..., :up.shape[-1]] |= up[..., :shape_bottom[1]]
        elif two:
            mask_bottom[..., :mask.shape[-1]] |= mask[..., :shape_bottom[1]]
        else:
            raise ValueError("a bottom-layer mask needs bottom_code and an index that holds bottom maps")
    return top_frame, bottom_frame, mask_top, mask_bottom, two


def similar_sounds(index, top_code: torch.Tensor, bottom_code: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None,
                   layer: str = 'top', start_index_top: int = 0, k: int = 8,
                   attribute_constraints: Optional[Mapping[str, object]] = None):
    """The k items of a `utils.datasets.code_index.CodeIndex` nearest to a sound, as a list of
    ((top [1,F_t,T_t], bottom [1,F_b,T_b]), attributes, distance), nearest first (equal distances by item index).
    top_code [1,F_t,T], bottom_code [1,F_b,T_b] or None (the top layer alone is compared): the query is the window of the
    stored duration starting at `start_index_top`, cut as `timerange_change` cuts its model window; a map shorter than the
    stored duration is continued with its last column (`resize_codemaps_repeat_last`) and the added columns weigh nothing.
    mask bool [1,F,W] in the resolution of `layer` over the window: True = do not compare here ("the sounds that agree
    with everything outside my hole"); a top-layer mask extends to the bottom layer as `timerange_change` extends it.
    attribute_constraints: `sample_from_database`'s.  The comparison runs on the device (csrc/code_search.hip)."""
    window = _similar_window(index, _one_map(top_code), _one_map(bottom_code), mask, layer, start_index_top)
    return _search_window(index, index.search, window, k=k, attribute_constraints=attribute_constraints)


def _fragment_window(index, top_code, bottom_code, start_index_top, width_top, mask, layer: str):
    """What `similar_fragments` compares, for maps whose last two dimensions are [F, T]:
    (query_top, query_bottom or None, mask_top, mask_bottom, two)."""
    _check_layer(layer)
    two = bottom_code is not None and index.bottom_shape is not None
    start, width = int(start_index_top), int(width_top)
    if start < 0 or width < 1 or start + width > top_code.shape[-1]:
        raise ValueError(f"the window [{start}, {start + width}) lies outside the top map's {top_code.shape[-1]} columns")
    device = index.device
    ratio_t = index.bottom_shape[1] // index.top_shape[1] if two else 1
    ratio_f = index.bottom_shape[0] // index.top_shape[0] if two else 1
    query_top = top_code[..., start:start + width]
    query_bottom = bottom_code[..., ratio_t * start:ratio_t * (start + width)] if two else None
    mask_top = mask_bottom = None
    if mask is not None:
        mask = mask.to(device).reshape(1, *mask.shape[-2:])
        want = (index.top_shape[0], width) if layer == 'top' else ((index.bottom_shape[0], ratio_t * width) if two else None)
        if want is None:
            raise ValueError("a bottom-layer mask needs bottom_code and an index that holds bottom maps")
        if mask.dtype != torch.bool or tuple(mask.shape[-2:]) != want:
            raise ValueError(f"mask: expected bool [1, {want[0]}, {want[1]}] over the window in the {layer} layer's "
                             f"resolution, got {mask.dtype} {tuple(mask.shape)}")
        if layer == 'top':
            mask_top = mask
            if two:
                mask_bottom = _bottom_mask(mask, ratio_f, ratio_t)
        else:
            mask_bottom = mask
    return query_top, query_bottom, mask_top, mask_bottom, two


def similar_fragments(index, top_code: torch.Tensor, bottom_code: Optional[torch.Tensor], start_index_top: int, width_top: int,
                      mask: Optional[torch.Tensor] = None, layer: str = 'top', k: int = 8,
                      shift_range: Optional[Tuple[int, int]] = None,
                      attribute_constraints: Optional[Mapping[str, object]] = None):
    """The k items of a `CodeIndex` that contain something nearest to a FRAGMENT of a sound, wherever it sits in time, as a
    list of ((top [1,F_t,T_t], bottom [1,F_b,T_b]), attributes, distance, shift_top), nearest first (equal distances by
    item index).  The query is the `width_top` top columns of the sound starting at `start_index_top` (and the matching
    bottom columns, cut with the ratio `similar_sounds` uses); shift_top is the item's column under the window's first one.
    mask bool [1,F,W] in the resolution of `layer` over that window: True = do not compare here; a top-layer mask extends to
    the bottom layer as `timerange_change` extends it.  shift_range=(lo, hi): only offsets lo <= o < hi of the stored
    maps.  The comparison runs on the device (`CodeIndex.search_shifted`, csrc/code_shift_search.hip)."""
    window = _fragment_window(index, _one_map(top_code), _one_map(bottom_code), start_index_top, width_top, mask, layer)
    return _search_window(index, index.search_shifted, window, k=k, shift_range=shift_range,
                          attribute_constraints=attribute_constraints)


def _vector_maps(z: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Per-cell vectors [1, F, T, D] laid out as the windows cut them: [1, D, F, T]."""
    return None if z is None else z.reshape(1, *z.shape[-3:]).permute(0, 3, 1, 2)


def _similar_to_vectors(index, z_top: torch.Tensor, z_bottom: Optional[torch.Tensor], mask, layer: str, start_index_top: int,
                        k: int, attribute_constraints):
    """`similar_sounds` for per-cell vectors z_top [1, F_t, T, D], z_bottom [1, F_b, T_b, D] or None: the same window, the
    same masks, `CodeIndex.search_soft` in place of `search`."""
    window = _similar_window(index, _vector_maps(z_top), _vector_maps(z_bottom), mask, layer, start_index_top)
    return _search_window(index, index.search_soft, window, vectors=True, k=k, attribute_constraints=attribute_constraints)


@torch.no_grad()
def similar_sounds_to_spectrogram(index, vqvae, spectrogram: torch.Tensor, mask: Optional[torch.Tensor] = None,
                                  layer: str = 'top', k: int = 8, start_index_top: int = 0, two_layers: bool = True,
                                  attribute_constraints: Optional[Mapping[str, object]] = None):
    """`similar_sounds` for a sound that is not in the database -- an upload: spectrogram [1, C, H, W] on the GPU is
    encoded to the vectors the codebook search sees (`VQVAE.encode_vectors`) and those, NOT the codes they would snap to,
    are compared with the stored codes' vectors: dist = sum_c w[c] |z[c] - E[x[c]]|^2 (`CodeIndex.search_soft`, DESIGN.md
    section 6c.2), so the upload's quantisation error is not counted as signal.  mask, layer, start_index_top, k,
    attribute_constraints and the returned list are `similar_sounds`'s; two_layers=False compares the top layer alone."""
    z_top, z_bottom, _, _ = vqvae.encode_vectors(spectrogram)
    if z_top.shape[0] != 1:
        raise ValueError(f"one sound per call: the spectrogram holds {z_top.shape[0]}")
    return _similar_to_vectors(index, z_top, z_bottom if two_layers else None, mask, layer, start_index_top, k,
                               attribute_constraints)


@torch.no_grad()
def similar_to_mixture(index, vqvae, codes_t: torch.Tensor, weights_t: torch.Tensor, codes_b: Optional[torch.Tensor] = None,
                       weights_b: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, layer: str = 'top',
                       k: int = 8, start_index_top: int = 0, attribute_constraints: Optional[Mapping[str, object]] = None):
    """The stored sounds nearest to a MORPH, without snapping it to codes: codes_* int64 and weights_* fp32 [M, 1, F, T] as
    `decode_code_mix` takes them (`morph`, `crossfade`, `VQVAE.encode_topm` with `soft_weights`); each cell's vector is
    the mixture sum_m weights[m] E[codes[m]] (`QuantizedBottleneck.embed_mix`) and is compared with the stored codes'
    vectors (`CodeIndex.search_soft`).  codes_b None: the top layer alone.  One-hot weights give `similar_sounds` on the
    codes they select, bit for bit.  mask, layer, start_index_top, k, attribute_constraints and the returned list are
    `similar_sounds`'s."""
    z_top = vqvae.quantize_t.embed_mix(codes_t, weights_t)
    z_bottom = None if codes_b is None else vqvae.quantize_b.embed_mix(codes_b, weights_b)
    if z_top.shape[0] != 1:
        raise ValueError(f"one sound per call: the mixture holds {z_top.shape[0]}")
    return _similar_to_vectors(index, z_top, z_bottom, mask, layer, start_index_top, k, attribute_constraints)


@torch.no_grad()
def similar_fragments_to_spectrogram(index, vqvae, spectrogram: torch.Tensor, start_index_top: int, width_top: int,
                                     mask: Optional[torch.Tensor] = None, layer: str = 'top', k: int = 8,
                                     shift_range: Optional[Tuple[int, int]] = None, two_layers: bool = True,
                                     attribute_constraints: Optional[Mapping[str, object]] = None):
    """`similar_fragments` for an upload: the window of `width_top` top columns from `start_index_top` on is cut from the
    encoder's vectors (`VQVAE.encode_vectors`) and laid over every stored sound at every offset that fits
    (`CodeIndex.search_shifted_soft`).  The other arguments and the returned list -- ((top, bottom), attributes, distance,
    shift_top) -- are `similar_fragments`'s."""
    z_top, z_bottom, _, _ = vqvae.encode_vectors(spectrogram)
    if z_top.shape[0] != 1:
        raise ValueError(f"one sound per call: the spectrogram holds {z_top.shape[0]}")
    window = _fragment_window(index, _vector_maps(z_top), _vector_maps(z_bottom if two_layers else None), start_index_top,
                              width_top, mask, layer)
    return _search_window(index, index.search_shifted_soft, window, vectors=True, k=k, shift_range=shift_range,
                          attribute_constraints=attribute_constraints)


def _paste_indexed(sound: torch.Tensor, item: torch.Tensor, mask: torch.Tensor, columns: torch.Tensor,
                   source: torch.Tensor) -> torch.Tensor:
    """sound [1,F,T] with the cells under mask [1,F,len(columns)] taken from item [1,F,T_i]: sound column columns[c] from
    item column source[c]; columns outside the sound or the item stay as they are."""
    sound = sound.clone()
    inside = (columns >= 0) & (columns < sound.shape[-1]) & (source >= 0) & (source < item.shape[-1])
    chosen = mask.to(sound.device)[..., inside.to(sound.device)]
    columns, source = columns[inside].to(sound.device), source[inside].to(sound.device)
    sound[..., columns] = torch.where(chosen, item.to(sound.device, sound.dtype)[..., source], sound[..., columns])
    return sound


def _paste_layers(top_code, bottom_code, item_top, item_bottom, mask, layer: str, columns_of, width_top: Optional[int] = None):
    """What `paste_fragment` and `paste_warped` share: the maps and the mask as [1,F,T]; `layer`, the mask's type, its rows
    and -- where the window's width in top columns is known -- its columns checked (ValueError); then the paste of both
    layers for a top-layer mask, which extends to the bottom layer as `timerange_change` extends it, and of the bottom
    layer alone for a bottom-layer mask.  columns_of(W, scale) -> (sound columns, item columns) under a mask of W columns
    of a layer that has `scale` columns per top column."""
    _check_layer(layer)
    top_code, bottom_code, item_top, item_bottom, mask = (_one_map(m) for m in (top_code, bottom_code, item_top, item_bottom,
                                                                                mask))
    ratio_t, ratio_f = bottom_code.shape[-1] // top_code.shape[-1], bottom_code.shape[-2] // top_code.shape[-2]
    rows = top_code.shape[-2] if layer == 'top' else bottom_code.shape[-2]
    width = None if width_top is None else width_top * (1 if layer == 'top' else ratio_t)
    if mask.dtype != torch.bool or mask.shape[-2] != rows or width not in (None, mask.shape[-1]):
        raise ValueError(f"mask: expected bool [1, {rows}, {'W' if width is None else width}] in the {layer} layer's "
                         f"resolution, got {mask.dtype} {tuple(mask.shape)}")
    if layer == 'top':
        top_code = _paste_indexed(top_code, item_top, mask, *columns_of(mask.shape[-1], 1))
        mask = _bottom_mask(mask, ratio_f, ratio_t)
    else:
        top_code = top_code.clone()
    return top_code, _paste_indexed(bottom_code, item_bottom, mask, *columns_of(mask.shape[-1], ratio_t))


def paste_fragment(top_code: torch.Tensor, bottom_code: torch.Tensor, item_top: torch.Tensor, item_bottom: torch.Tensor,
                   mask: torch.Tensor, layer: str, window_start_top: int, shift_top: int):
    """Fill a hole with a retrieved sound's codes: the cells of (top_code [1,F_t,T], bottom_code [1,F_b,T_b]) under
    mask bool [1,F,W] -- in the resolution of `layer`, over the window that starts at top column `window_start_top` -- take
    the codes of (item_top, item_bottom), sound column `col` from item column `col - window_start_top + shift_top` (in
    bottom columns: both scaled by the time ratio).  A top-layer mask extends to the bottom layer as `timerange_change`
    extends it; a bottom-layer mask leaves the top map alone.  Cells whose source column falls outside the item stay
    unchanged.  Pure indexing: works on CPU tensors.  Returns the new (top, bottom)."""
    def columns_of(W, scale):                        # the mask's own width: any number of bottom columns for a bottom mask
        start, shift = int(window_start_top), int(shift_top)
        columns = torch.arange(W) + scale * start
        return columns, columns + scale * (shift - start)
    return _paste_layers(top_code, bottom_code, item_top, item_bottom, mask, layer, columns_of)


def similar_sounds_warped(index, top_code: torch.Tensor, bottom_code: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None,
                          layer: str = 'top', start_index_top: int = 0, k: int = 8, drift: Tuple[int, int] = (-4, 4),
                          attribute_constraints: Optional[Mapping[str, object]] = None):
    """`similar_sounds` for sounds that unfold a little faster or slower than the query: the same window, masks and returned
    list, compared by `CodeIndex.search_warped` -- every query column is matched to one item column, the item's time may
    hold, step or skip from one query column to the next, and its drift against the query stays in drift=(lo, hi) top
    columns.  `CodeIndex.warp_paths` gives the alignment of a returned item, `paste_warped` copies
    codes along it."""
    window = _similar_window(index, _one_map(top_code), _one_map(bottom_code), mask, layer, start_index_top)
    return _search_window(index, index.search_warped, window, k=k, drift=drift, attribute_constraints=attribute_constraints)


def paste_warped(top_code: torch.Tensor, bottom_code: torch.Tensor, item_top: torch.Tensor, item_bottom: torch.Tensor,
                 mask: torch.Tensor, start_index_top: int, path, layer: str = 'top'):
    """`paste_fragment` along a warped alignment: path [W] (`CodeIndex.warp_paths`) names, for the query column i that sits
    at top column `start_index_top` + i of the sound, the item's top column p(i).  The cells under mask bool [1,F,W] (in
    the resolution of `layer`; r W columns for the bottom layer) take the item's codes: top column start + i from item
    column p(i), bottom columns r (start + i) + u from r p(i) + u, u < r.  A top-layer mask extends to the bottom layer as
    in `paste_fragment`; columns outside the sound or the item stay as they are.  With path[i] = o + i this is
    `paste_fragment` at shift_top = o, bit for bit.  Pure indexing: works on CPU tensors.  Returns the new (top, bottom)."""
    _check_layer(layer)
    path = torch.as_tensor(path).reshape(-1).to('cpu', torch.int64)

    def columns_of(W, scale):                        # every top column of the path as its `scale` columns of the layer
        columns, fine = torch.arange(len(path)) + int(start_index_top), torch.arange(scale)
        return tuple((scale * c[:, None] + fine[None, :]).reshape(-1) for c in (columns, path))
    return _paste_layers(top_code, bottom_code, item_top, item_bottom, mask, layer, columns_of, width_top=len(path))


def patch_from_database(index, top_code: torch.Tensor, bottom_code: torch.Tensor, mask: torch.Tensor, layer: str = 'top',
                        context_top: int = 4, k: int = 1, attribute_constraints: Optional[Mapping[str, object]] = None):
    """Fill a hole from the code database instead of sampling it: mask bool [1,F,T] in the resolution of `layer` over the
    WHOLE sound, its masked columns are the hole.  The query is the window from `context_top` top columns before the hole to
    `context_top` after it, clipped to the sound, with the hole masked -- "agree with what surrounds my hole, anywhere in
    time" (`similar_fragments`); each of the k nearest items is pasted into the hole at its best offset (`paste_fragment`).
    Returns a list of ((top [1,F_t,T], bottom [1,F_b,T_b]), attributes, distance, shift_top), nearest first."""
    _check_layer(layer)
    top_code, bottom_code, mask = _one_map(top_code), _one_map(bottom_code), _one_map(mask)
    whole = top_code if layer == 'top' else bottom_code
    if mask.dtype != torch.bool or tuple(mask.shape[-2:]) != tuple(whole.shape[-2:]):
        raise ValueError(f"mask: expected bool [1, {whole.shape[-2]}, {whole.shape[-1]}] over the whole {layer} map, got "
                         f"{mask.dtype} {tuple(mask.shape)}")
    holed = mask.any(-2).reshape(-1).nonzero().reshape(-1)
    if holed.numel() == 0:
        raise ValueError("mask: nothing is masked, there is no hole to fill")
    ratio_t = bottom_code.shape[-1] // top_code.shape[-1]
    first, last = int(holed[0]), int(holed[-1]) + 1                  # the hole's columns [first, last) in `layer`
    if layer == 'bottom':
        first, last = first // ratio_t, -(-last // ratio_t)
    start = max(0, first - int(context_top))
    width = min(top_code.shape[-1], last + int(context_top)) - start
    scale = 1 if layer == 'top' else ratio_t
    window_mask = mask[..., scale * start:scale * (start + width)]
    out = []
    for (item_top, item_bottom), attributes, distance, shift in similar_fragments(
            index, top_code, bottom_code, start, width, mask=window_mask, layer=layer, k=k,
            attribute_constraints=attribute_constraints):
        if item_bottom is None:
            raise ValueError("patch_from_database: the index holds no bottom maps")
        patched = paste_fragment(top_code, bottom_code, item_top, item_bottom, window_mask, layer, start, shift)
        out.append((patched, attributes, distance, shift))
    return out


MORPH_MAX_SOURCES = 8          # sources of one mixture (isi_embed_mix_f32)
MORPH_SWEEP_MAX_STEPS = 256    # rows of one sweep: the batch cap of native sampling (priors/_decode.py)


def _morph_codes(sounds) -> Tuple[torch.Tensor, torch.Tensor]:
    """M (top_code, bottom_code) pairs of equal shapes -> int64 stacks ([M, B, F_t, T_t], [M, B, F_b, T_b])."""
    sounds = list(sounds)
    if not 1 <= len(sounds) <= MORPH_MAX_SOURCES:
        raise ValueError(f"morph mixes 1 to {MORPH_MAX_SOURCES} sounds, got {len(sounds)}")
    tops, bottoms = [], []
    for top, bottom in sounds:
        if top.dim() < 2 or bottom.dim() < 2:
            raise ValueError("a sound is a (top_code [B, F_t, T_t], bottom_code [B, F_b, T_b]) pair")
        tops.append(top.reshape(-1, *top.shape[-2:]))
        bottoms.append(bottom.reshape(-1, *bottom.shape[-2:]))
    for name, maps in (("top", tops), ("bottom", bottoms)):
        if any(m.shape != maps[0].shape or m.dtype != torch.int64 or m.device != maps[0].device for m in maps):
            raise ValueError(f"the sounds' {name} codemaps must be int64 maps of one shape on one device")
    top, bottom = torch.stack(tops), torch.stack(bottoms)
    if top.shape[1] != bottom.shape[1] or bottom.shape[2] % top.shape[2] or bottom.shape[3] % top.shape[3]:
        raise ValueError(f"bottom maps {tuple(bottom.shape[1:])} are not a refinement of the top maps {tuple(top.shape[1:])}")
    return top, bottom


def _morph_weights(weights, M: int, F: int, T: int, name: str) -> torch.Tensor:
    """M scalars, [M, T] or [M, F, T] -> fp32 [M, F, T] on the host, checked as the kernel will see it: finite,
    non-negative, summing to 1 over the sources within 1e-6 in every cell."""
    w = weights.detach().cpu() if isinstance(weights, torch.Tensor) else torch.as_tensor(weights)
    w = w.to(torch.float64)
    if w.dim() == 1 and w.shape[0] == M:
        w = w.reshape(M, 1, 1)
    elif w.dim() == 2 and tuple(w.shape) == (M, T):
        w = w.reshape(M, 1, T)
    elif not (w.dim() == 3 and tuple(w.shape) == (M, F, T)):
        raise ValueError(f"{name}: expected {M} scalars, [{M}, {T}] or [{M}, {F}, {T}], got {tuple(w.shape)}")
    w = w.expand(M, F, T).to(torch.float32)
    if not bool(torch.isfinite(w).all()):
        raise ValueError(f"{name}: weights must be finite")
    if bool((w < 0).any()):
        raise ValueError(f"{name}: weights must be non-negative")
    if bool(((w.double().sum(0) - 1).abs() > 1e-6).any()):
        raise ValueError(f"{name}: the weights of every cell must sum to 1 (within 1e-6)")
    return w.contiguous()


def _check_mixed_codes(codes: torch.Tensor, weights: torch.Tensor, n_embed: int, name: str) -> None:
    # one device sync, skipped while a HIP graph is being captured (like QuantizedBottleneck.embed_code)
    if codes.is_cuda and torch.cuda.is_current_stream_capturing():
        return
    if bool((((codes < 0) | (codes >= n_embed)) & (weights != 0)).any()):
        raise IndexError(f"{name} code out of range under a non-zero weight")


def _snap_to_codes(bottleneck, quant: torch.Tensor) -> torch.Tensor:
    """quant [B, H, W, D] -> ids [B, H, W] by the bottleneck's eval-mode nearest-code search (no codebook update)."""
    was_training = bottleneck.training
    bottleneck.eval()
    try:
        return bottleneck(quant)[2]
    finally:
        bottleneck.train(was_training)


def _mix(vqvae, codes_t, weights_t, codes_b, weights_b, snap: bool):
    """codes / weights [M, B, F, T] per level, the weights already checked: the spectrogram, or the snapped codemaps."""
    weights_t, weights_b = weights_t.to(codes_t.device), weights_b.to(codes_b.device)
    _check_mixed_codes(codes_t, weights_t, vqvae.quantize_t.n_embed, "top")
    _check_mixed_codes(codes_b, weights_b, vqvae.quantize_b.n_embed, "bottom")
    if not snap:
        return vqvae.decode_code_mix(codes_t, weights_t, codes_b, weights_b)
    return (_snap_to_codes(vqvae.quantize_t, vqvae.quantize_t.embed_mix(codes_t, weights_t)),
            _snap_to_codes(vqvae.quantize_b, vqvae.quantize_b.embed_mix(codes_b, weights_b)))


@torch.no_grad()
def morph(vqvae, sounds, weights, weights_bottom=None, snap: bool = False):
    """Render a mixture of sounds: in every cell of both codemaps the decoder receives sum_m w[m] * E[code_m] instead of one
    codebook row (`VQVAE.decode_code_mix`, csrc/code_mix.hip).

    `sounds`: M <= 8 (top_code [B, F_t, T_t], bottom_code [B, F_b, T_b]) pairs of equal shapes.  `weights`, in top
    resolution: M scalars ("70 % of this, 30 % of that"), [M, T_t] -- one weight per source and top column, a morph that
    moves in time -- or [M, F_t, T_t].  Every top cell's weight is repeated over the bottom cells under it unless
    `weights_bottom` gives the bottom map its own (the same three forms in bottom resolution).  The weights are host
    values: finite, non-negative and summing to 1 per cell within 1e-6, anything else raises ValueError -- a convex mix
    stays inside the codebook's hull and therefore inside the decoder's operand range.  A zero weight hides its code (the
    priors' mask token may sit under it); a code outside the codebook under a non-zero weight raises IndexError (one
    device sync, skipped during stream capture, where the cell decodes to NaN instead).

    Returns the spectrogram, as `decode_code` does.  `snap`: instead the (top_code, bottom_code) nearest to the mixed maps
    (each bottleneck's eval-mode search): a sound the priors, the search and the UI can go on editing."""
    codes_t, codes_b = _morph_codes(sounds)
    M, B = codes_t.shape[:2]
    w_t = _morph_weights(weights, M, *codes_t.shape[2:], "weights")
    if weights_bottom is None:
        w_b = w_t.repeat_interleave(codes_b.shape[2] // codes_t.shape[2], 1).repeat_interleave(codes_b.shape[3] // codes_t.shape[3], 2)
    else:
        w_b = _morph_weights(weights_bottom, M, *codes_b.shape[2:], "weights_bottom")
    w_t = w_t.unsqueeze(1).expand(M, B, *w_t.shape[1:]).contiguous()
    w_b = w_b.unsqueeze(1).expand(M, B, *w_b.shape[1:]).contiguous()
    return _mix(vqvae, codes_t, w_t, codes_b, w_b, snap)


@torch.no_grad()
def morph_sweep(vqvae, a, b, steps: int) -> torch.Tensor:
    """`steps` spectrograms [steps, C, H, W] from sound `a` to sound `b` ((top_code [1, F_t, T_t], bottom_code
    [1, F_b, T_b]) each): row s mixes (1 - alpha_s) a + alpha_s b at alpha = linspace(0, 1, steps), as `morph` with those
    two scalars would.  One batch, one decode call; at most 256 steps."""
    steps = int(steps)
    if not 1 <= steps <= MORPH_SWEEP_MAX_STEPS:
        raise ValueError(f"morph_sweep: steps must be 1..{MORPH_SWEEP_MAX_STEPS}, got {steps}")
    codes_t, codes_b = _morph_codes([a, b])
    if codes_t.shape[1] != 1:
        raise ValueError("morph_sweep: a and b are single sounds (batch 1)")
    alpha = torch.linspace(0, 1, steps, dtype=torch.float32)
    w = torch.stack([1 - alpha, alpha]).reshape(2, steps, 1, 1)          # (1 - alpha) + alpha = 1 within one rounding
    codes_t, codes_b = (c.expand(2, steps, *c.shape[2:]).contiguous() for c in (codes_t, codes_b))
    return _mix(vqvae, codes_t, w.expand(codes_t.shape).contiguous(), codes_b, w.expand(codes_b.shape).contiguous(), False)


@torch.no_grad()
def crossfade(vqvae, a, b, start_index_top: int, width_top: int, snap: bool = False):
    """Sound `a` before top column `start_index_top`, sound `b` from column `start_index_top + width_top` on, and between
    them a linear ramp in the latent: ramp column j of n carries (j + 1) / (n + 1) of `b`, with n = `width_top` columns in
    the top map and, finer, n = ratio * `width_top` columns in the bottom map.  `width_top` = 0 is the hard cut: the decode
    of the spliced codemaps, bit for bit.  Returns what `morph` returns."""
    codes_t, codes_b = _morph_codes([a, b])
    start, width = int(start_index_top), int(width_top)
    T = codes_t.shape[3]
    if start < 0 or width < 0 or start + width > T:
        raise ValueError(f"crossfade: window [{start}, {start + width}) does not lie inside the {T} top columns")

    def ramp(columns: int, scale: int) -> torch.Tensor:
        j = torch.arange(columns, dtype=torch.float64) - scale * start
        wb = ((j + 1) / (scale * width + 1)).clamp(0, 1)
        return torch.stack([1 - wb, wb])

    return morph(vqvae, [a, b], ramp(T, 1), ramp(codes_b.shape[3], codes_b.shape[3] // T), snap=snap)


@torch.no_grad()
def render_with_palette(vqvae, spectrogram: torch.Tensor, palette_top, palette_bottom=None):
    """Quantise `spectrogram` [B, C, H, W] with another sound's codes: (top_code [B, F_t, T_t], bottom_code [B, F_b, T_b]),
    in every cell the nearest code of the level's palette -- typically `sample.codes_in_use(other_top, K)` and
    `sample.codes_in_use(other_bottom, K)`, bool rows [K]; any single palette `VQVAE.encode_topm` takes will do.
    `palette_bottom` None leaves the bottom level unrestricted.  The bottom level is searched under the top map the
    palette produced.  The results are ordinary codemaps for the priors, the search and `decode_code`.  An empty palette
    raises ValueError (a cell would have no code)."""
    K_t, K_b = vqvae.quantize_t.n_embed, vqvae.quantize_b.n_embed

    def one_palette(p, K, name):
        if p is None:
            return None
        t = torch.as_tensor(p)
        row = t.reshape(-1).cpu() if t.dtype == torch.bool else None
        if row is None:                                       # code indices
            idx = t.reshape(-1).long().cpu()
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= K):
                raise ValueError(f"render_with_palette: {name} holds a code outside [0, {K})")
            row = torch.zeros(K, dtype=torch.bool)
            row[idx] = True
        if row.shape[0] != K:
            raise ValueError(f"render_with_palette: {name} must be a bool row [{K}] or a tensor of code indices")
        if not bool(row.any()):
            raise ValueError(f"render_with_palette: {name} allows no code")
        return row

    codes_t, _, codes_b, _ = vqvae.encode_topm(spectrogram, m=1, allowed_codes_top=one_palette(palette_top, K_t, "palette_top"),
                                               allowed_codes_bottom=one_palette(palette_bottom, K_b, "palette_bottom"))
    return codes_t[0], codes_b[0]


@torch.no_grad()
def encode_soft(vqvae, spectrogram: torch.Tensor, m: int, temperature: float):
    """One sound as per-cell mixtures of its `m` nearest codes: (codes_t, weights_t, codes_b, weights_b), each
    [m, B, F, T] of its level, ready for `VQVAE.decode_code_mix` (and, a source at a time, for `morph`).  The weights are
    `VQVAE.soft_weights` of the codebook distances: softmax of -(d_m - d_0) / temperature; temperature 0 puts weight 1 on
    the nearest code, and the decode is then `decode_code` of the hard codemaps bit for bit."""
    codes_t, dist_t, codes_b, dist_b = vqvae.encode_topm(spectrogram, m=m)
    return codes_t, vqvae.soft_weights(dist_t, temperature), codes_b, vqvae.soft_weights(dist_b, temperature)


@torch.no_grad()
def code_alternatives(vqvae, spectrogram: torch.Tensor, m: int, layer: str):
    """"What else could stand here?" by the VQ-VAE's own metric: (ids int64 [m, B, F, T], distances fp32 [m, B, F, T]) of
    `layer` ('top' or 'bottom'), nearest first -- rank 0 is the cell's own code, the others are the swaps that stay closest
    to the recorded sound.  (`sample.codemap_statistics` gives the prior's alternatives.)"""
    if layer not in ('top', 'bottom'):
        raise ValueError(f"layer must be 'top' or 'bottom', got {layer!r}")
    codes_t, dist_t, codes_b, dist_b = vqvae.encode_topm(spectrogram, m=m)
    return (codes_t, dist_t) if layer == 'top' else (codes_b, dist_b)


def sample_from_database(codes_dataset, label_encoders_per_modality: Mapping[str, object], duration_top: int,
                         attribute_constraints: Mapping[str, object], generator: Optional[torch.Generator] = None, *,
                         similar_to: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None, index=None):
    """The lookup of `/sample-from-dataset` (flask_server.py:333-372): items of the code database
    (`utils.datasets.lmdb_dataset.LMDBDataset`: (top [F_t,T_t], bottom [F_b,T_b], {class name: tensor [1]})) are visited in
    a random order until one meets every constraint -- equality on the decoded attributes, `pitch_class` = pitch % 12 and
    `octave` = pitch // 12 derived from the pitch (the reference stores the octave under the `pitch_class` key, :351-353,
    so its octave constraint can never be met; the evident intent is built here).  The reference draws with replacement
    for ever; a database without a match raises LookupError here.  Returns ((top [1,F_t,T], bottom [1,F_b,T_b]), attributes).
    similar_to=(top, bottom) with index=a `CodeIndex` of the database: the item NEAREST to that sound among those meeting
    the constraints (`similar_sounds`, k = 1) instead of a random one; `codes_dataset` and `generator` are then not read."""
    if (similar_to is None) != (index is None):
        raise ValueError("sample_from_database: similar_to=(top, bottom) and index=CodeIndex go together")
    if index is not None:
        (top_code, bottom_code), attributes, _ = similar_sounds(index, similar_to[0], similar_to[1], k=1,
                                                                attribute_constraints=attribute_constraints)[0]
        if bottom_code is None:
            raise ValueError("sample_from_database: the index holds no bottom maps")
        return resize_codemaps_repeat_last(top_code, bottom_code, duration_top), attributes
    for index in torch.randperm(len(codes_dataset), generator=generator).tolist():
        top_code, bottom_code, encoded = codes_dataset[index]
        attributes = {key: label_encoders_per_modality[key].inverse_transform([int(torch.as_tensor(value).reshape(-1)[0])])[0]
                      for key, value in encoded.items()}
        if 'pitch' in attributes:
            attributes['pitch_class'] = int(attributes['pitch']) % 12
            attributes['octave'] = int(attributes['pitch']) // 12
        if all(key in attributes and attributes[key] == wanted for key, wanted in attribute_constraints.items()):
            top_code, bottom_code = torch.as_tensor(top_code).unsqueeze(0), torch.as_tensor(bottom_code).unsqueeze(0)
            return resize_codemaps_repeat_last(top_code, bottom_code, duration_top), attributes
    raise LookupError(f"no item of the code database meets {dict(attribute_constraints)}")


# nine samples of the viridis colour map (0, 1/8, .. 1), interpolated linearly: the map the reference draws with
_VIRIDIS = ((68, 1, 84), (71, 44, 122), (59, 81, 139), (44, 113, 142), (33, 144, 141), (39, 173, 129), (92, 200, 99),
            (170, 220, 50), (253, 231, 37))


def _png_bytes(rgb: torch.Tensor) -> bytes:
    """[H, W, 3] uint8 -> PNG (8-bit truecolour, one IDAT chunk; standard library only)."""
    h, w, _ = rgb.shape
    rows = torch.cat([torch.zeros(h, 1, dtype=torch.uint8), rgb.reshape(h, w * 3)], 1)      # filter type 0 per scanline

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(rows.numpy().tobytes(), 6)) + chunk(b"IEND", b""))


@torch.no_grad()
def spectrogram_png(vqvae, top_code: torch.Tensor, bottom_code: torch.Tensor, upsampling_factor: int = 1) -> bytes:
    """The compute of `/get-spectrogram-image` (flask_server.py:103-143, 1024-1046): decode the codes, take the
    log-magnitude channel of the first item, upsample it bilinearly, and draw it full-frame in viridis with the lowest
    frequency at the bottom and the colour range spanning the map's own minimum .. maximum (what `specshow` does).  The
    reference rasterises through matplotlib at 2400 x 1600; here one pixel per (upsampled) spectrogram bin."""
    s = vqvae.decode_code(top_code, bottom_code)[0, 0].float()
    if upsampling_factor > 1:
        s = torch.nn.functional.interpolate(s[None, None], mode='bilinear', scale_factor=upsampling_factor)[0, 0]
    s = s.flip(0).cpu()
    lo, hi = float(s.min()), float(s.max())
    t = ((s - lo) / (hi - lo) if hi > lo else torch.zeros_like(s)).clamp(0, 1) * (len(_VIRIDIS) - 1)
    i0 = t.floor().long().clamp(max=len(_VIRIDIS) - 2)
    lut = torch.tensor(_VIRIDIS, dtype=torch.float32)
    frac = (t - i0).unsqueeze(-1)
    rgb = (lut[i0] * (1 - frac) + lut[i0 + 1] * frac).round().to(torch.uint8)
    return _png_bytes(rgb)
