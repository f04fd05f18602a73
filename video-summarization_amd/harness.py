"""Training and evaluation harness: the counterparts of the reference's ``train_step`` (``src/train.py:111-131``, on packed
ragged batches: ``train_step_packed``), of ``pretrain.py``'s step (``src/pretrain.py:49-86``, on packed ragged batches:
``pretrain_step_packed``) and of ``val_step`` (``src/train.py:134-152``).  ``train_epoch_resident`` / ``pretrain_epoch_resident``
are the same epochs over a device-resident ``data.TrainSet`` / ``data.PretrainSet``: no loader, no host collate, no
per-step ``loss.item()``.

``val_step(model, loader, device)`` keeps the reference's contract: ``loader`` yields
``(feature [1,T,1024], target [1,T], user)`` per video (reference ``collate_fn_test``,
``data/dataset.py:164-168``), the model is called unchanged, ``sigmoid`` is applied by the caller and
the per-video scores go to ``eval_metrics`` keyed by ``user.name``.  Returns
``(mean MSE loss, f_score, kendall_tau, spearman_r)`` like the reference.

``val_step_batched`` is the MI355X-friendly form of the same computation: the videos are scored in
length-bucketed padded batches (optionally sharded over ranks, scores gathered with one all_gather) and the
result is bit-identical per frame, because a video's scores do not depend on the batch it is scored in.
"""
from __future__ import annotations

from typing import Iterable, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from .corpus import packed_scorer, plan_shards, score_corpus
from .evaluation import eval_metrics, eval_videos
from .losses import mse_packed_loss, mse_with_mask_loss


def train_step_packed(model, optim, loader: Iterable, scaler, device):
    """The reference's ``train_step`` (``src/train.py:111-131``) on PACKED batches: ``loader`` yields ``(feature [sum T_i, 1024],
    target [sum T_i], lengths)`` (``data.collate_fn_train_packed``); no sentinel rows, no mask, the same loss value and
    gradients as the padded step.  Any ``torch.optim`` optimizer or the native ``Adam``; an unmodified ``GradScaler``.
    Returns the mean loss over the batches."""
    model.train()
    total, n = 0.0, 0
    for feature, target, lengths in loader:
        feature, target = feature.to(device), target.to(device)
        with torch.amp.autocast("cuda"):                                    # train.py:120
            pred, _ = model.forward_packed_train(feature, lengths)
            loss = mse_packed_loss(pred, target, lengths)                   # train.py:122
        optim.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(optim)
        scaler.update()
        total, n = total + loss.item(), n + 1
    return total / max(n, 1)


def pretrain_step_packed(model, optimizer, schedular, scaler, loader: Iterable, device):
    """The reference's pretraining step (``src/pretrain.py:49-86``) on PACKED batches: ``loader`` yields ``(feature [sum T_i,
    1024], vid_rep [B, 512], lengths)`` (``data.collate_fn_pretrain_packed``); no sentinel rows and no mask, the same losses
    and gradients as the padded step (``PretrainModel.forward_packed``).  Any ``torch.optim`` optimizer or the native
    ``Adam``; an unmodified ``GradScaler``; ``schedular.update()`` after every step unless ``schedular`` is None.  Returns the
    mean loss over the batches."""
    model.train()
    total, n = 0.0, 0
    for feature, vid_rep, lengths in loader:
        feature, vid_rep = feature.to(device), vid_rep.to(device)
        with torch.amp.autocast("cuda"):                                    # pretrain.py:59
            main_loss, center_loss, repel_loss = model.forward_packed(feature, vid_rep, lengths)
            loss = main_loss + center_loss * 0.5 + 1. * repel_loss          # pretrain.py:62
        optimizer.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(optimizer)
        scaler.update()
        if schedular is not None:
            schedular.update()
        total, n = total + loss.item(), n + 1
    return total / max(n, 1)


def _mean_of_steps(losses: torch.Tensor, n: int) -> float:
    """The number the loader loops return: the steps' fp32 losses (ONE device-to-host copy) added in step order as Python
    floats, divided by their count; 0.0 for an epoch without a batch."""
    total = 0.0
    for v in (losses.tolist() if n else []):
        total += v
    return total / max(n, 1)


def train_epoch_resident(model, optim, train_set, scaler, batch_size, packed: bool = True, shuffle: bool = True,
                         drop_last: bool = False):
    """One fine-tuning epoch over a ``data.TrainSet``: the body of ``train_step_packed`` (``packed=False``: of the reference's
    ``train_step`` with the padded forward and ``mse_with_mask_loss``) on batches cut on the device - the batches, order,
    generator draws and therefore the result of ``DataLoader(ds, shuffle=shuffle, batch_size=batch_size, drop_last=drop_last)``
    with the matching collate, bit for bit.  Each step's loss is stored in a device vector and read back once, after the
    epoch.  Returns the mean loss over the batches."""
    model.train()
    batches = train_set.epoch(batch_size, shuffle=shuffle, drop_last=drop_last, packed=packed)
    n = len(batches)
    losses = torch.empty((n,), dtype=torch.float32, device=train_set.device)
    for i, (feature, target, third) in enumerate(batches):
        with torch.amp.autocast("cuda"):                                    # train.py:120
            if packed:                                                      # third: lengths
                pred, _ = model.forward_packed_train(feature, third)
                loss = mse_packed_loss(pred, target, third)
            else:                                                           # third: the padding mask of train.py:118
                pred, _ = model(feature, third)
                loss = mse_with_mask_loss(pred, target, third)              # train.py:122
        optim.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(optim)
        scaler.update()
        losses[i].copy_(loss.detach())
    return _mean_of_steps(losses, n)


def pretrain_epoch_resident(model, optimizer, schedular, scaler, pretrain_set, batch_size, packed: bool = True):
    """One pretraining epoch over a ``data.PretrainSet``: the body of ``pretrain_step_packed`` (``packed=False``: the padded
    ``PretrainModel.forward`` with the mask of ``pretrain.py:57``) on batches cut on the device, shuffled with
    ``drop_last=True`` as ``pretrain.py:18-25`` builds its loader; ``schedular.update()`` after every step unless ``schedular``
    is None.  Losses are read back once, after the epoch.  Returns the mean loss over the batches."""
    model.train()
    batches = pretrain_set.epoch(batch_size, shuffle=True, drop_last=True, packed=packed)
    n = len(batches)
    losses = torch.empty((n,), dtype=torch.float32, device=pretrain_set.device)
    for i, (feature, vid_rep, third) in enumerate(batches):
        with torch.amp.autocast("cuda"):                                    # pretrain.py:59
            if packed:
                main_loss, center_loss, repel_loss = model.forward_packed(feature, vid_rep, third)
            else:
                main_loss, center_loss, repel_loss = model(feature, vid_rep, third)
            loss = main_loss + center_loss * 0.5 + 1. * repel_loss          # pretrain.py:62
        optimizer.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(optimizer)
        scaler.update()
        if schedular is not None:
            schedular.update()
        losses[i].copy_(loss.detach())
    return _mean_of_steps(losses, n)


@torch.no_grad()
def val_step(model, loader: Iterable, device):
    model.eval()
    score_dict, user_dict = {}, {}
    loss_sum, n = 0.0, 0
    for feature, target, user in loader:
        feature, target = feature.to(device), target.to(device)
        pred, _ = model(feature)                                   # train.py:143
        pred = torch.sigmoid(pred.view(1, -1))                     # train.py:144
        loss_sum += F.mse_loss(pred, target).item()                # train.py:145-147
        n += 1
        score_dict[user.name] = pred.squeeze(0).detach().cpu().numpy()
        user_dict[user.name] = user
    f_score, ktau, spr = eval_metrics(score_dict, user_dict)       # train.py:150
    return loss_sum / max(n, 1), f_score, ktau, spr


def evaluate_shard(scores, targets, users, order):
    """[sum MSE loss, sum F-score, sum Kendall tau, sum Spearman rho] over the videos `order` (indices): the keyshot
    evaluation of a rank's shard as ONE library call (`evaluation.eval_videos` -> vs_eval_corpus: one bounded host thread
    pool over every video and every (video, user) pair), sums in index order."""
    if not order:
        return [0.0, 0.0, 0.0, 0.0]
    f, k, s = eval_videos({i: scores[i].numpy() for i in order}, {i: users[i] for i in order}, "avg")
    loss = 0.0
    for i in order:
        loss += F.mse_loss(scores[i].view(1, -1), targets[i].detach().float().cpu().view(1, -1)).item()
    return [loss, float(f.sum()), float(k.sum()), float(s.sum())]


def evaluate_shard_device(eval_set, flat, targets, order):
    """`evaluate_shard` from scores that never left the device: `flat` holds the scores of the videos `order`
    (ascending indices into the EvalSet) concatenated.  The keyshot evaluation is `EvalSet.evaluate`; the per-video MSE
    is taken on the device in float64 (one cumulative sum over the squared differences) and the four sums on the
    host, in index order, in double."""
    if not order:
        return [0.0, 0.0, 0.0, 0.0]
    f, k, s = eval_set.evaluate(flat, videos=[eval_set.keys[i] for i in order])
    tgt = [targets[i].detach().reshape(-1) for i in order]
    tgt = (torch.cat(tgt) if len(tgt) > 1 else tgt[0]).to(device=flat.device, dtype=torch.float32)
    ends = torch.tensor([t.numel() for t in (targets[i] for i in order)], dtype=torch.int64).cumsum(0)
    total = torch.cat([torch.zeros(1, dtype=torch.float64, device=flat.device), (flat - tgt).double().square().cumsum(0)])
    ends_d = ends.to(flat.device)
    starts_d = torch.cat([torch.zeros(1, dtype=torch.int64, device=flat.device), ends_d[:-1]])
    per_video = ((total[ends_d] - total[starts_d]) / (ends_d - starts_d).double()).cpu()
    loss = 0.0
    for x in per_video.tolist():
        loss += x
    return [loss, float(np.sum(f)), float(np.sum(k)), float(np.sum(s))]


@torch.no_grad()
def val_step_batched(model, features: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], users: Sequence,
                     device, rank: int = 0, world: int = 1, group=None, max_frames: int = 65536, eval_set=None):
    """Same result as ``val_step`` over (features[i] [T_i,1024], targets[i] [T_i], users[i]).

    ``eval_set``: an ``evaluation.EvalSet`` built over ``users`` (same order).  Each rank then evaluates the videos it
    scored from the scores still on its device (no score all-gather, no score device-to-host copy), takes the MSE loss
    there too, and only the all-reduce of the four sums stays.  F-score, tau and rho are the default path's bit for bit."""
    model.eval()
    packed_fn = packed_scorer(model)      # PACKED batches where the model has them (no sentinel padding, no mask; the same bits)
    if eval_set is not None:
        order, flat = score_corpus(lambda x, m: model.score(x, m), list(features), rank=rank, world=world, group=group,
                                   device=device, max_frames=max_frames, packed_fn=packed_fn, keep_on_device=True)
        sums = evaluate_shard_device(eval_set, flat, targets, order)
        return _reduce_sums(sums, len(users), device, world, group)
    scores = score_corpus(lambda x, m: model.score(x, m), list(features), rank=rank, world=world, group=group,
                          device=device, max_frames=max_frames, packed_fn=packed_fn)
    # every rank holds every video's scores; the (CPU) evaluation is sharded too: a rank evaluates the videos it
    # scored and the four sums are all-reduced.  Sums run in a fixed per-rank order.
    lengths = [int(f.shape[0]) for f in features]
    mine = plan_shards(lengths, world)[rank] if world > 1 else list(range(len(users)))
    order = sorted(mine)

    sums = evaluate_shard(scores, targets, users, order)
    return _reduce_sums(sums, len(users), device, world, group)


def _reduce_sums(sums, n_videos, device, world, group):
    """All-reduce of a rank's [loss, F-score, tau, rho] sums, then the means over the corpus."""
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor(sums, dtype=torch.float64,
                         device=device if (device is not None and dist.get_backend(group) == "nccl") else "cpu")
        dist.all_reduce(t, group=group)
        sums = t.tolist()
    n = max(n_videos, 1)
    return sums[0] / n, sums[1] / n, sums[2] / n, sums[3] / n
