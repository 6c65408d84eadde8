"""Float64 definition of the population BatchNorm statistics (engine/precise_bn.py, sfod_bn_finalize_pop, sfod_bn_pop_commit,
sfod_bn_pop_merge), numpy only.

A pass hands a layer ``nblocks`` block statistics per channel -- count n_b, sum s_b, centred square sum m2_b (about the
block's own mean) -- exactly what the convolution's epilogue writes as fp32.  The definition

  * merges the blocks of a pass pairwise by Chan's update into (M, mu_b, tot)       ``merge_blocks``
  * merges the passes the same way into the accumulator (n, mean, M2)                ``chan_merge``
  * commits running_mean = fp32(mean), running_var = fp32(M2 / n)  (biased)          ``commit``

all in float64 with one rounding at the end.  ``fault`` plants one of the two classic mistakes, so that a test can show
that its comparison would catch them: "unweighted" averages the passes' means and variances without their sizes,
"unbiased" divides by n - 1.

``fvcore_population`` is the estimator of fvcore's ``update_bn_stats`` as published (``_PopulationVarianceEstimator``), fed
with per-pass (mean, unbiased variance, M): batch second moment = mean^2 + var (M - 1) / M, running means weighted by
M / total, pop_var = E[x^2] - E[x]^2."""
import numpy as np


def block_stats(x, bounds):
    """x [M, C] float64 samples, ``bounds`` the block edges (0 = b_0 <= b_1 <= ... = M; equal edges: an empty block)
    -> fp32 (counts [nb], sums [nb, C], m2 [nb, C]) like a convolution epilogue writes them"""
    nb = len(bounds) - 1
    C = x.shape[1]
    counts = np.zeros(nb, np.float32)
    sums = np.zeros((nb, C), np.float32)
    m2 = np.zeros((nb, C), np.float32)
    for b in range(nb):
        blk = x[bounds[b]:bounds[b + 1]]
        counts[b] = len(blk)
        if len(blk):
            sums[b] = blk.sum(0)
            m2[b] = ((blk - blk.mean(0)) ** 2).sum(0)
    return counts, sums, m2


def chan_merge(a, b):
    """(n, mean, M2) of the union of two disjoint sets from theirs; n scalar or [C], mean / M2 [C]; float64"""
    na, ma, qa = (np.asarray(v, np.float64) for v in a)
    nb, mb, qb = (np.asarray(v, np.float64) for v in b)
    n = na + nb
    safe = np.where(n > 0, n, 1.0)
    d = mb - ma
    mean = ma + d * nb / safe
    m2 = qa + qb + d * d * na * nb / safe
    return n, mean, m2


def merge_blocks(counts, sums, m2):
    """fp32 block statistics of one pass -> (M, batch mean, batch centred square sum) in float64"""
    C = sums.shape[1]
    acc = (np.zeros(C), np.zeros(C), np.zeros(C))
    for b in range(len(counts)):
        nb = float(counts[b])
        if nb > 0:
            acc = chan_merge(acc, (np.full(C, nb), sums[b].astype(np.float64) / nb, m2[b].astype(np.float64)))
    return acc


def accumulate(passes, fault=None):
    """``passes``: (M, mu_b, tot) per pass (``merge_blocks``) -> accumulator (n, mean, M2)"""
    if fault == "unweighted":
        # the older rule: plain average of the per-pass means and (biased) variances
        means = np.stack([p[1] for p in passes])
        vars_ = np.stack([p[2] / p[0] for p in passes])
        n = sum(p[0] for p in passes)
        return n, means.mean(0), vars_.mean(0) * n
    C = len(passes[0][1])
    acc = (np.zeros(C), np.zeros(C), np.zeros(C))
    for p in passes:
        acc = chan_merge(acc, p)
    return acc


def commit(acc, fault=None):
    """accumulator -> (running_mean fp32, running_var fp32); columns with n = 0 come back as NaN ("not written")"""
    n, mean, m2 = acc
    div = n - 1.0 if fault == "unbiased" else n
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.where(n > 0, m2 / div, np.nan)
    return np.where(n > 0, mean, np.nan).astype(np.float32), var.astype(np.float32)


def fvcore_population(batch_means, batch_unbiased_vars, batch_sizes):
    """fvcore ``_PopulationVarianceEstimator`` over the passes, float64 -> (pop_mean, pop_var)"""
    tot = 0.0
    pop_mean = np.zeros_like(np.asarray(batch_means[0], np.float64))
    pop_sq = np.zeros_like(pop_mean)
    for m, v, M in zip(batch_means, batch_unbiased_vars, batch_sizes):
        m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
        sq = m * m + v * ((M - 1.0) / M)
        tot += M
        pop_mean += (m - pop_mean) * (M / tot)
        pop_sq += (sq - pop_sq) * (M / tot)
    return pop_mean, pop_sq - pop_mean * pop_mean


def mean_gate(mu, var, bits):
    """2^-bits (|mu| + sigma)"""
    return 2.0 ** -bits * (np.abs(mu) + np.sqrt(var))
