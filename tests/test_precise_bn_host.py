"""TEST.PRECISE_BN without a GPU: the float64 definition (tests/helpers/precise_bn_definitions.py) against numpy.mean /
numpy.var of the concatenated samples, the two planted faults, and the host logic of engine/precise_bn.py and the trainer's
hook (period rule, module selection, NUM_ITER, no loader for a model without live BatchNorm)."""
import types

import numpy as np
import pytest
import torch

from helpers import precise_bn_definitions as D


def _passes(seed=0, C=5, sizes=(37, 5, 160), offset=0.0):
    rng = np.random.default_rng(seed)
    xs = [rng.normal(offset + rng.normal(size=C) * 0.5, 0.5 + rng.random(C), size=(m, C)) for m in sizes]
    out = []
    for x in xs:
        cuts = sorted(rng.integers(0, len(x) + 1, size=3).tolist())
        out.append(D.merge_blocks(*D.block_stats(x, [0] + cuts + [cuts[-1], len(x)])))     # one empty block among them
    return xs, out


def _errors(xs, passes, fault_acc=None, fault_commit=None):
    """worst error / gate of (mean, var): gates 2^-23 (|mu| + sigma) and 2^-22 var, the kernel tests' own"""
    allx = np.concatenate(xs)
    mu, var = allx.mean(0), allx.var(0)
    rm, rv = D.commit(D.accumulate(passes, fault=fault_acc), fault=fault_commit)
    return (np.abs(rm - mu) / D.mean_gate(mu, var, 23)).max(), (np.abs(rv - var) / (2.0 ** -22 * var)).max()


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_definition_is_the_statistics_of_the_concatenated_samples(offset):
    xs, passes = _passes(offset=offset)
    assert float(passes[0][0][0]) == 37 and float(passes[2][0][0]) == 160
    em, ev = _errors(xs, passes)
    # block statistics are fp32 (2^-24 relative each): the mean carries that on |mu|, a cancelling variance on sum / M, which
    # at |mu| = 1000 sigma is no longer inside the fp32 gates -- there the definition is compared in float64 below
    if offset == 0.0:
        assert em < 1.0 and ev < 1.0, (em, ev)
    # float64 block statistics: the merge itself is exact to double rounding
    acc = D.accumulate([D.chan_merge((np.zeros(5), np.zeros(5), np.zeros(5)),
                                     (np.full(5, float(len(x))), x.mean(0), ((x - x.mean(0)) ** 2).sum(0))) for x in xs])
    allx = np.concatenate(xs)
    np.testing.assert_allclose(acc[1], allx.mean(0), rtol=1e-13)
    np.testing.assert_allclose(acc[2] / acc[0], allx.var(0), rtol=1e-9 if offset else 1e-12)


def test_planted_faults_are_caught():
    xs, passes = _passes()
    em, ev = _errors(xs, passes, fault_acc="unweighted")
    assert em > 1e3 and ev > 1e3, (em, ev)           # means and variances of 5 rows weigh as much as those of 160
    em, ev = _errors(xs, passes, fault_commit="unbiased")
    assert em < 1.0 and ev > 1e3, (em, ev)           # 1 / (N - 1) against 1 / N at N = 202: 5e-3 relative


def test_fvcore_estimator_agrees_with_the_definition():
    xs, passes = _passes()
    pm, pv = D.fvcore_population([x.mean(0) for x in xs], [x.var(0, ddof=1) for x in xs], [len(x) for x in xs])
    allx = np.concatenate(xs)
    np.testing.assert_allclose(pm, allx.mean(0), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(pv, allx.var(0), rtol=1e-10)


def test_a_layer_that_never_ran_is_not_written():
    rm, rv = D.commit((np.array([0.0, 4.0]), np.array([0.0, 1.0]), np.array([0.0, 8.0])))
    assert np.isnan(rm[0]) and np.isnan(rv[0]) and rm[1] == 1.0 and rv[1] == 2.0


# ---- host logic ------------------------------------------------------------------------------------------------------------
def test_period_rule(sfod):
    due = sfod.engine.precise_bn.precise_bn_due
    assert [n for n in range(1, 5) if due(n, 4, 0)] == [4]                   # EVAL_PERIOD 0: after the last iteration only
    assert [n for n in range(1, 5) if due(n, 4, 2)] == [2, 4]
    assert [n for n in range(1, 6) if due(n, 5, 2)] == [2, 4, 5]             # the final iteration off the period as well
    assert [n for n in range(1, 4) if due(n, 10, 0)] == []


def _toy_model(sfod):
    from importlib import import_module
    rn = import_module("simple-sfod_amd.modeling.backbone_resnet")
    live, evalbn = torch.nn.BatchNorm2d(4), torch.nn.BatchNorm2d(4)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), live, evalbn, rn.FrozenBatchNorm2d(4), torch.nn.GroupNorm(2, 4))
    m.train()
    evalbn.eval()
    return m, live


def test_get_bn_modules_takes_live_batchnorm_only(sfod):
    m, live = _toy_model(sfod)
    got = sfod.engine.precise_bn.get_bn_modules(m)
    assert len(got) == 1 and got[0] is live
    m.eval()
    assert sfod.engine.precise_bn.get_bn_modules(m) == []


class _Stub:
    """what ``BaseTrainer._build_precise_bn`` touches of a trainer"""

    def __init__(self, model):
        self.model, self.built = model, 0

    def build_train_loader(self, cfg):
        self.built += 1
        return iter(())


def _cfg(sfod, *opts):
    return sfod.config.setup_cfg(None, ["OUTPUT_DIR", ""] + list(opts))


def test_num_iter_below_one_raises_naming_the_key(sfod):
    m, _ = _toy_model(sfod)
    build = sfod.engine.BaseTrainer._build_precise_bn
    for bad in ("0", "-3"):
        with pytest.raises(ValueError, match="TEST.PRECISE_BN.NUM_ITER"):
            build(_Stub(m), _cfg(sfod, "TEST.PRECISE_BN.ENABLED", "True", "TEST.PRECISE_BN.NUM_ITER", bad))
    with pytest.raises(ValueError, match="TEST.PRECISE_BN.NUM_ITER"):
        sfod.engine.precise_bn.update_bn_stats(m, [], 0)
    st = _Stub(m)
    build(st, _cfg(sfod, "TEST.PRECISE_BN.NUM_ITER", "0"))          # not enabled: the key is not read
    assert st.built == 0 and st._precise_bn_loader is None


def test_enabled_builds_a_second_loader_only_for_live_batchnorm(sfod):
    build = sfod.engine.BaseTrainer._build_precise_bn
    m, _ = _toy_model(sfod)
    st = _Stub(m)
    build(st, _cfg(sfod, "TEST.PRECISE_BN.ENABLED", "True"))
    assert st.built == 1 and st._precise_bn_loader is not None and st._precise_bn_iter is None
    frozen = _Stub(torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.GroupNorm(2, 4)).train())
    build(frozen, _cfg(sfod, "TEST.PRECISE_BN.ENABLED", "True"))
    assert frozen.built == 0 and frozen._precise_bn_loader is None
    off = _Stub(m)
    build(off, _cfg(sfod))
    assert off.built == 0 and off._precise_bn_loader is None
    assert _cfg(sfod).SFOD.PRECISE_BN.SYNC is False


def test_batch_selection(sfod):
    pb = sfod.engine.precise_bn
    plain = types.SimpleNamespace()
    strong, weak = [{"image": 0}], [{"image": 1}]
    assert pb.frames_of(plain, weak) == [weak]                               # a labelled loader's list
    assert pb.frames_of(plain, (strong, weak)) == [weak]                     # two crops: the weak half
    assert pb.frames_of(plain, (strong, weak, strong, strong)) == [weak]     # four lists: data[1], as adabn_refinement
    da = object.__new__(sfod.modeling.da_faster_rcnn.DAFasterRCNN)
    assert pb.frames_of(da, (strong, weak)) == [strong, weak]                # (source, target): both, source first
