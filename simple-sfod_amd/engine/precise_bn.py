"""``TEST.PRECISE_BN``: population BatchNorm statistics (Detectron2's ``hooks.PreciseBN`` over fvcore's
``update_bn_stats``; the reference's trainers put the hook between the LR scheduler and the checkpointer, base.py:237-245).

After ``num_iters`` train-mode forward passes under ``no_grad`` every live BatchNorm layer's ``running_mean`` /
``running_var`` hold the statistics of ALL elements it saw in those passes: per channel, with M_p rows in pass p,

    N = sum_p M_p,   mu = sum x / N,   var = sum (x - mu)^2 / N   (biased),

the size-weighted rule of fvcore's ``_PopulationVarianceEstimator`` (batch second moment mean^2 + var (M - 1) / M, running
means weighted by M / total, var = E[x^2] - E[x]^2) evaluated in float64 and rounded once.  The statistics pass costs no
launch of its own: the BatchNorm finalize of each layer merges its batch into an fp64 accumulator by Chan's update
(sfod_bn_finalize_pop) instead of moving the running buffers, and one launch writes all layers' buffers at the end
(sfod_bn_pop_commit).  As in fvcore ``num_batches_tracked`` grows by one per pass, ``momentum`` and every parameter stay, the
running buffers are written only at the end."""
import itertools

import torch
import torch.distributed as dist

from .. import native


def get_bn_modules(model):
    """fvcore ``get_bn_modules``: the BatchNorm2d modules in training mode (eval-mode modules and FrozenBatchNorm2d, which
    is not a BatchNorm2d, hold fixed statistics and are left out)."""
    return [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d) and m.training]


def precise_bn_due(next_iter, max_iter, eval_period):
    """Detectron2's ``PreciseBN.after_step``: after the last iteration and every ``eval_period`` iterations (0: last only)."""
    return next_iter == max_iter or (eval_period > 0 and next_iter % eval_period == 0)


def validate_num_iter(num_iter):
    if int(num_iter) < 1:
        raise ValueError(f"TEST.PRECISE_BN.NUM_ITER must be at least 1, got {num_iter}")
    return int(num_iter)


def frames_of(model, data):
    """What of one loader batch passes the backbone for the statistics -> list of frame lists.  A two-crop batch
    ``(strong, weak)`` gives its weak half (``adabn_refinement`` takes ``data[1]`` too; of a four-list batch that is the weak
    labelled half); a ``DALoader`` batch ``(source, target)`` gives both, source first: ``DAFasterRCNN`` runs its backbone on
    both."""
    if not isinstance(data, tuple):
        return [data]
    from ..modeling.da_faster_rcnn import DAFasterRCNN
    if isinstance(model, DAFasterRCNN) and len(data) == 2:
        return [data[0], data[1]]
    return [data[1]]


def _backbones(model):
    return [m for m in model.modules() if hasattr(m, "bn_population") and hasattr(m, "forward_nhwc")]


@torch.no_grad()
def update_bn_stats(model, batches, num_iters, sync=False):
    """``num_iters`` batches of ``batches`` (an iterable or iterator; an iterator is left where the last batch ended) through
    ``model.preprocess_image`` + ``model._features`` -> population statistics in every live BatchNorm of the model's
    backbone(s).  ``sync``: with more than one rank, the ranks' accumulators are gathered and merged in rank order before the
    commit, so that every rank holds the statistics of the union; False: each rank its own share.  -> number of layers."""
    num_iters = validate_num_iter(num_iters)
    backbones = _backbones(model)
    owned = {id(m) for bb in backbones for m in bb.modules()}
    bns = [m for m in get_bn_modules(model) if id(m) in owned]
    if not bns:
        return 0
    acc, views = native.bn_pop_accumulator([bn.num_features for bn in bns], bns[0].running_mean.device)
    table = dict(zip(bns, views))
    try:
        for bb in backbones:
            bb.bn_population = table
        for data in itertools.islice(batches, num_iters):
            for frames in frames_of(model, data):
                model._features(model.preprocess_image(frames))
        if sync and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            acc = _merge_over_ranks(acc)
        offs = list(itertools.accumulate([0] + [bn.num_features for bn in bns[:-1]]))
        native.bn_pop_commit(acc, [(o, bn.running_mean, bn.running_var) for o, bn in zip(offs, bns)])
    finally:
        for bb in backbones:
            bb.bn_population = None
    return len(bns)


def _merge_over_ranks(acc):
    """all-gather of the accumulators, merged 0, 1, ... on every rank: the same operands in the same order, the same bits"""
    staged = acc.cpu() if dist.get_backend() == "gloo" else acc      # gloo gathers host tensors only
    parts = [torch.empty_like(staged) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, staged)
    out = torch.zeros_like(acc)
    for p in parts:
        native.bn_pop_merge(out, p.to(acc.device))
    return out
