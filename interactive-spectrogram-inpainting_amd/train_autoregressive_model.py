"""Training / validation epoch of the transformer prior on MI355X
(reference train_autoregressive_model.py:119-372 `run_model`).

Same loop semantics: per batch of `(top, bottom, class_conditioning)` code maps

  hier == 'top', self-conditional : source = target = top, inpainting mask from `mask_sampler`
                                    applied to the source side              (:178-205)
  hier == 'bottom'                : target = bottom, condition = top         (:218-231)
  logits -> time-frequency map with the class dim on axis 1                  (:233-234)
  loss = criterion(logits_map, target)  (LabelSmoothingLoss)                 (:254)
  backward, optional clip_grad_norm_, optimizer.step(), scheduler.step()     (:256-263)
  accuracy = mean(argmax == target); satisfied-constraints count             (:265-273)
  returns (loss_sum, total_accuracy, num_samples)  sample-weighted           (:372)

What differs by design: the reference wraps the model in `nn.DataParallel` (:145);
here data parallelism is one process per GPU (torch.distributed "nccl" = RCCL) with
`GradBucketReducer` averaging gradients bucket by bucket while the backward is still
running.  Forward and backward of every heavy operator are HIP kernels
(priors/_train.py); plotting / TensorBoard are out of scope.
"""
from __future__ import annotations

import argparse
import time
from typing import Iterable, Optional

import torch
import torch.distributed as dist

from interactive_spectrogram_inpainting.priors.sequence_mask import SequenceMask
from interactive_spectrogram_inpainting.priors.transformer import VQNSynthTransformer
from interactive_spectrogram_inpainting.utils.distributed import GradBucketReducer, is_distributed
from interactive_spectrogram_inpainting.utils.training.optimizer import DeviceHyperAdam, clip_and_step, make_adam


def num_satisfied_constraints(predicted: torch.Tensor, condition: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Positions where the prediction keeps the unmasked (given) codes (reference :104-116)."""
    correct = torch.eq(predicted, condition).float()
    return torch.masked_fill(correct, mask, 1).sum()


def run_model(args, epoch: int, loader: Iterable, model: VQNSynthTransformer, optimizer, scheduler, device,
              criterion, tensorboard_writer=None, is_training: bool = True,
              mask_sampler: Optional[SequenceMask] = None, clip_grad_norm: Optional[float] = None,
              reducer: Optional[GradBucketReducer] = None, hip_graph: bool = False):
    """One epoch.  `args.hier` in {'top', 'bottom'}.  With torch.distributed initialised each rank
    runs its own shard of the data and `reducer` (built once over model.parameters()) averages the
    gradients; the returned sums are this rank's.  `hip_graph`: a training epoch replays one recorded
    step (`_run_training_epoch_graphed`)."""
    if hip_graph and is_training:
        return _run_training_epoch_graphed(args, epoch, loader, model, optimizer, scheduler, device, criterion,
                                           mask_sampler, clip_grad_norm, reducer)
    hier = args.hier
    model.train(is_training)
    loss_sum, total_accuracy, num_samples = 0.0, 0.0, 0
    satisfied_total = 0.0 if model.self_conditional_model else None
    if is_training and reducer is None and is_distributed() and dist.get_world_size() > 1:
        raise RuntimeError("distributed training needs a GradBucketReducer")

    for top, bottom, class_conditioning_tensors in loader:
        if is_training:
            if reducer is not None:
                reducer.zero()
            else:
                optimizer.zero_grad(set_to_none=True)
        class_conditioning_tensors = {k: v.to(device, non_blocking=True).view(-1, 1)
                                      for k, v in class_conditioning_tensors.items()}
        top = top.to(device, non_blocking=True)
        mask = None
        with torch.set_grad_enabled(is_training):
            if hier == 'top':
                if not model.self_conditional_model:
                    raise NotImplementedError("the unconditional top model is not built (see priors/transformer.py)")
                kind, source, target = 'target', top, top
                # the sampler draws in sequence order [B,S]; the wrapper wants the time-frequency layout
                mask = model.to_time_frequency_map(mask_sampler.sample_mask(top.shape[0]).to(device), kind='source')
                source_sequence, target_sequence = model.to_sequences(
                    target, condition=source, class_conditioning=class_conditioning_tensors, mask=mask)
            elif hier == 'bottom':
                kind, target = 'target', bottom.to(device, non_blocking=True)
                source_sequence, target_sequence = model.to_sequences(
                    target, condition=top, class_conditioning=class_conditioning_tensors)
            else:
                raise ValueError(f"unknown hierarchy level {hier}")
            logits_sequence, _ = model(target_sequence, condition=source_sequence)
            logits_map = model.to_time_frequency_map(logits_sequence, kind=kind, permute_output_as_logits=True)
            loss = criterion(logits_map, target)

        if is_training:
            loss.backward()
            if reducer is not None:
                reducer.finish()
            clip_and_step(model.parameters(), optimizer, clip_grad_norm)
            if scheduler is not None:
                scheduler.step()

        with torch.no_grad():
            pred = logits_map.argmax(1)
            accuracy = (pred == target).float().mean()
            batch = top.shape[0]
            if model.self_conditional_model:
                satisfied_total += float(num_satisfied_constraints(pred, source, mask))
            loss_sum += float(loss) * batch          # (joins the device: the step's deferred index verdict has arrived too)
            total_accuracy += float(accuracy) * batch
            num_samples += batch
        if is_training:
            # the training path gathers on clamped indices and defers the range verdict (priors/transformer.py embed_data):
            # raise the reference's IndexError here, where the loss was read back anyway -- before the next optimizer step
            # trains on another clamped symbol
            model.check_indices()
    if tensorboard_writer is not None and not is_training:
        tensorboard_writer.add_scalar(f'code_prediction-validation_{hier}/mean_loss', loss_sum / max(1, num_samples), epoch)
        tensorboard_writer.add_scalar(f'code_prediction-validation_{hier}/mean_accuracy',
                                      total_accuracy / max(1, num_samples), epoch)
    model.check_indices()       # (end of the epoch: nothing pending may outlive it, e.g. into a checkpoint)
    run_model.last_satisfied_constraints = satisfied_total
    return loss_sum, total_accuracy, num_samples


class GraphedPriorStep:
    """The training branch of `run_model`'s loop body recorded into HIP graph segments (utils/training/graphed_step.py) and
    replayed per batch.  Static inputs: the target codemap, the mask (top) or the top codemap (bottom), and the class
    tensors in sorted key order.  The sample-weighted loss / accuracy / satisfied-constraint sums are accumulated by the
    recording itself into `sums` (float64, on the device) and read once per epoch.  Like GraphedVQVAEStep, the model and
    the optimizer's state are put back in place after the recording's eager warm-up steps.  The optimizer is a
    DeviceHyperAdam (replays follow `param_groups`) or a capturable one (constant learning rate)."""

    def __init__(self, hier: str, model: VQNSynthTransformer, optimizer, criterion, statics, class_keys, clip_grad_norm,
                 reducer):
        from interactive_spectrogram_inpainting import _hip
        from interactive_spectrogram_inpainting.utils.training.graphed_step import GraphedTrainingStep
        self.sums = torch.zeros(3, dtype=torch.float64, device=statics[0].device)
        self.class_keys = list(class_keys)
        batch = statics[0].shape[0]

        def step(target, other, *cls):
            if reducer is not None:
                reducer.zero()
            else:
                optimizer.zero_grad(set_to_none=True)
            class_conditioning = dict(zip(self.class_keys, cls))
            if hier == 'top':
                source = target
                source_sequence, target_sequence = model.to_sequences(
                    target, condition=source, class_conditioning=class_conditioning, mask=other)
            else:
                source_sequence, target_sequence = model.to_sequences(
                    target, condition=other, class_conditioning=class_conditioning)
            logits_sequence, _ = model(target_sequence, condition=source_sequence)
            logits_map = model.to_time_frequency_map(logits_sequence, kind='target', permute_output_as_logits=True)
            loss = criterion(logits_map, target)
            loss.backward()
            if reducer is not None:
                reducer.finish()
            clip_and_step(model.parameters(), optimizer, clip_grad_norm)
            with torch.no_grad():
                pred = logits_map.argmax(1)
                accuracy = (pred == target).float().mean()
                satisfied = (num_satisfied_constraints(pred, target, other) if model.self_conditional_model
                             else torch.zeros((), device=target.device))
                self.sums += torch.stack([loss.detach().double() * batch, accuracy.double() * batch, satisfied.double()])
            return loss.detach()

        tensors = list(model.parameters()) + list(model.buffers())
        saved = [t.detach().clone() for t in tensors]
        had_state = {id(p) for p in optimizer.state}
        saved_opt = {id(p): {k: v.detach().clone() for k, v in st.items() if torch.is_tensor(v)}
                     for p, st in optimizer.state.items()}
        saved_steps = [g.get("step") for g in optimizer.param_groups]
        device_hyper = isinstance(optimizer, DeviceHyperAdam)
        limits = {0: model.n_class_target}
        if hier == 'bottom':
            limits[1] = model.n_class_source
        for i, k in enumerate(self.class_keys):
            limits[2 + i] = model.class_conditioning_num_classes_per_modality[k]
        self.graphed = GraphedTrainingStep(step, [t.clone() for t in statics], warmup=2, index_limits=limits,
                                           range_params=[p for p in model.parameters() if p.dim() == 2],
                                           optimizers=[optimizer] if device_hyper else None)
        with torch.no_grad():       # the warm-up steps trained on the first batch: put everything back IN PLACE
            for t, sv in zip(tensors, saved):
                t.copy_(sv)
            for p_, st in optimizer.state.items():
                for k, v in st.items():
                    if torch.is_tensor(v):
                        v.copy_(saved_opt[id(p_)][k]) if id(p_) in had_state else v.zero_()
            self.sums.zero_()
        if device_hyper:
            for g, n in zip(optimizer.param_groups, saved_steps):
                g["step"] = n
        _hip._on_optimizer_step()      # (values moved without a version bump: caches keyed on versions are stale)

    def __call__(self, *batch: torch.Tensor) -> None:
        self.graphed(*batch)

    def finish(self) -> None:
        self.graphed.finish()


def _run_training_epoch_graphed(args, epoch, loader, model, optimizer, scheduler, device, criterion, mask_sampler,
                                clip_grad_norm, reducer):
    """`run_model(is_training=True)` with the step replayed from a recording.  The order is the eager loop's: the step runs
    with what `param_groups` holds, then `scheduler.step()`.  The recording is kept on the model across epochs; a batch
    of another size than the recorded one (a ragged last batch) runs as one eager step with the same optimizer.  Symbols
    outside their embedding tables raise the reference's IndexError (GraphedTrainingStep's `index_limits`)."""
    hier = args.hier
    if scheduler is not None and not isinstance(optimizer, DeviceHyperAdam):
        raise NotImplementedError("a recorded step bakes the learning rate in: a host-side scheduler with hip_graph needs "
                                  "make_adam(..., device_hyper=True)")
    if hier == 'top' and not model.self_conditional_model:
        raise NotImplementedError("the unconditional top model is not built (see priors/transformer.py)")
    if hier not in ('top', 'bottom'):
        raise ValueError(f"unknown hierarchy level {hier}")
    if reducer is None and is_distributed() and dist.get_world_size() > 1:
        raise RuntimeError("distributed training needs a GradBucketReducer")
    model.train(True)
    key = (id(optimizer), id(criterion), hier, clip_grad_norm, id(reducer))
    cached = getattr(model, "_graphed_train_step", None)
    graphed = cached[1] if cached is not None and cached[0][:5] == key else None
    if cached is not None and graphed is None:
        cached[1].finish()
        model._graphed_train_step = None
    loss_sum, total_accuracy, num_samples, satisfied_total = 0.0, 0.0, 0, 0.0
    ok = False
    try:
        for top, bottom, class_conditioning_tensors in loader:
            class_keys = sorted(class_conditioning_tensors)
            cls = [class_conditioning_tensors[k].to(device, non_blocking=True).view(-1, 1) for k in class_keys]
            top = top.to(device, non_blocking=True)
            if hier == 'top':
                # the sampler draws in sequence order [B,S]; the wrapper wants the time-frequency layout
                mask_sequence = mask_sampler.sample_mask(top.shape[0])
                mask = model.to_time_frequency_map(mask_sequence.to(device), kind='source')
                statics = (top, mask, *cls)
            else:
                statics = (bottom.to(device, non_blocking=True), top, *cls)
            shapes = tuple(tuple(t.shape) for t in statics)
            if graphed is not None and shapes != cached[0][5]:
                # one eager step with the same optimizer (and the mask already drawn for this batch)
                fixed = _FixedMask(mask_sequence) if hier == 'top' else mask_sampler
                ls, acc, n = run_model(args, epoch, [(top, bottom, class_conditioning_tensors)], model, optimizer, scheduler,
                                       device, criterion, is_training=True, mask_sampler=fixed,
                                       clip_grad_norm=clip_grad_norm, reducer=reducer)
                loss_sum, total_accuracy, num_samples = loss_sum + ls, total_accuracy + acc, num_samples + n
                satisfied_total += run_model.last_satisfied_constraints or 0.0
                continue
            if graphed is None:
                graphed = GraphedPriorStep(hier, model, optimizer, criterion, statics, class_keys, clip_grad_norm, reducer)
                cached = (key + (shapes,), graphed)
                model._graphed_train_step = cached
                graphed.sums.zero_()
            graphed(*statics)
            if scheduler is not None:
                scheduler.step()
            num_samples += top.shape[0]
        ok = True
    finally:
        if graphed is not None:
            try:
                graphed.finish()       # waits for the replays; raises a pending index / range verdict
            finally:
                if not ok:
                    model._graphed_train_step = None
    if graphed is not None:
        sums = graphed.sums.tolist()       # the epoch's one read-back
        graphed.sums.zero_()
        loss_sum, total_accuracy, satisfied_total = loss_sum + sums[0], total_accuracy + sums[1], satisfied_total + sums[2]
    model.check_indices()
    run_model.last_satisfied_constraints = satisfied_total if model.self_conditional_model else None
    return loss_sum, total_accuracy, num_samples


class _FixedMask:
    """A mask sampler that returns one mask already drawn (sequence order, as `SequenceMask.sample_mask` gives it)."""

    def __init__(self, mask_sequence: torch.Tensor):
        self.mask_sequence = mask_sequence

    def sample_mask(self, batch: int) -> torch.Tensor:
        return self.mask_sequence


class SyntheticCodes(torch.utils.data.Dataset):
    """Random code maps of the shapes `extract_code.py` writes (top [F_t,T_t], bottom [F_b,T_b])
    with NSynth-like class labels; stands in for the LMDB database (lmdb is not in this image)."""

    def __init__(self, n: int, top_shape, bottom_shape, n_class: int, classes_per_modality, seed: int = 0):
        g = torch.Generator().manual_seed(seed)
        self.top = torch.randint(0, n_class, (n, *top_shape), generator=g)
        self.bottom = torch.randint(0, n_class, (n, *bottom_shape), generator=g)
        self.cls = {k: torch.randint(0, v, (n,), generator=g) for k, v in classes_per_modality.items()}

    def __len__(self):
        return self.top.shape[0]

    def __getitem__(self, i):
        return self.top[i], self.bottom[i], {k: v[i] for k, v in self.cls.items()}


def main(argv=None):
    from interactive_spectrogram_inpainting.priors.sequence_mask import UniformProbabilityBernoulliSequenceMask
    from interactive_spectrogram_inpainting.priors.transformer import (SelfAttentiveVQTransformer,
                                                                      UpsamplingVQTransformer)
    from interactive_spectrogram_inpainting.utils.losses.prediction import LabelSmoothingLoss
    from interactive_spectrogram_inpainting.utils.training.scheduler import CycleScheduler

    ap = argparse.ArgumentParser(description="train the transformer prior on synthetic code maps")
    ap.add_argument('--hier', default='top', choices=['top', 'bottom'])
    ap.add_argument('--batch_size', type=int, default=8)
    ap.add_argument('--num_batches', type=int, default=4)
    ap.add_argument('--num_epochs', type=int, default=1)
    ap.add_argument('--lr', type=float, default=3e-4)
    ap.add_argument('--label_smoothing', type=float, default=0.0)
    ap.add_argument('--clip_grad_norm', type=float, default=None)
    ap.add_argument('--n_class', type=int, default=512)
    ap.add_argument('--top_shape', type=int, nargs=2, default=[32, 32])
    ap.add_argument('--num_encoder_layers', type=int, default=6)
    ap.add_argument('--num_decoder_layers', type=int, default=8)
    ap.add_argument('--hip_graph', action='store_true',
                    help="record the training step into HIP graph segments and replay it per batch; the optimizer is "
                         "then a DeviceHyperAdam, whose replays follow the scheduler")
    ap.add_argument('--database_path', default=None,
                    help="code database written by extract_code.py (LMDB, needs the `lmdb` package); "
                         "default: synthetic code maps")
    args = ap.parse_args(argv)

    distributed = 'RANK' in __import__('os').environ
    if distributed:
        dist.init_process_group('nccl')
        torch.cuda.set_device(int(__import__('os').environ.get('LOCAL_RANK', 0)))
    device = torch.device('cuda', torch.cuda.current_device())
    classes = {'pitch': 61, 'instrument_family_str': 11}
    common = dict(n_class=args.n_class, channel=8, kernel_size=5, n_block=1, n_res_block=1, res_channel=8,
                  use_relative_transformer=True, predict_frequencies_first=True, conditional_model=True,
                  class_conditioning_prepend_to_dummy_input=True,
                  class_conditioning_num_classes_per_modality=classes,
                  class_conditioning_embedding_dim_per_modality={k: 16 for k in classes},
                  conditional_model_num_encoder_layers=args.num_encoder_layers,
                  conditional_model_num_decoder_layers=args.num_decoder_layers)
    top_shape = list(args.top_shape)
    bottom_shape = [2 * top_shape[0], 2 * top_shape[1]]
    torch.manual_seed(2)
    if args.hier == 'top':
        model = SelfAttentiveVQTransformer(shape=top_shape, condition_shape=top_shape, self_conditional_model=True,
                                           add_mask_token_to_symbols=True, **common)
    else:
        model = UpsamplingVQTransformer(shape=bottom_shape, condition_shape=top_shape, **common)
    model = model.to(device)
    if args.database_path is not None:   # train_autoregressive_model.py:330-352 of the reference
        from interactive_spectrogram_inpainting.utils.datasets.lmdb_dataset import LMDBDataset
        data = LMDBDataset(args.database_path, classes_for_conditioning=list(classes))
        sampler_d = torch.utils.data.distributed.DistributedSampler(data) if distributed else None
        loader = torch.utils.data.DataLoader(data, batch_size=args.batch_size, shuffle=sampler_d is None, sampler=sampler_d)
    else:
        data = SyntheticCodes(args.batch_size * args.num_batches, top_shape, bottom_shape, args.n_class, classes,
                              seed=dist.get_rank() if distributed else 0)
        loader = torch.utils.data.DataLoader(data, batch_size=args.batch_size, shuffle=False)
    optimizer = make_adam(model.parameters(), lr=args.lr, device_hyper=args.hip_graph)
    scheduler = CycleScheduler(optimizer, args.lr, n_iter=len(loader) * args.num_epochs)
    criterion = LabelSmoothingLoss(args.n_class, args.label_smoothing, dim=1)
    reducer = GradBucketReducer(model.parameters()) if distributed else None
    sampler = UniformProbabilityBernoulliSequenceMask(
        low=0.0, high=1.0, sequence_duration=model.source_transformer_sequence_length,
        mask_token_index=model.mask_token_index) if args.hier == 'top' else None
    for epoch in range(args.num_epochs):
        torch.cuda.synchronize()
        t0 = time.time()
        loss_sum, acc_sum, n = run_model(args, epoch, loader, model, optimizer, scheduler, device, criterion,
                                         is_training=True, mask_sampler=sampler, clip_grad_norm=args.clip_grad_norm,
                                         reducer=reducer, hip_graph=args.hip_graph)
        torch.cuda.synchronize()
        if not distributed or dist.get_rank() == 0:
            print(f"epoch {epoch + 1}: loss {loss_sum / n:.5f} acc {acc_sum / n:.5f} "
                  f"{n / (time.time() - t0):.2f} samples/s/rank")
    if distributed:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
