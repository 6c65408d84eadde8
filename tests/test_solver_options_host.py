"""Host side of the solver options (engine/solver.py): WarmupCosineLR and the "constant" warm-up against the closed
forms, the scheduler dispatch, ValueError (never a bare assert) for what is not supported, and Detectron2's
``get_default_optimizer_params`` rule as a per-parameter table.  No GPU: FlatModelState runs on CPU tensors, and a
FusedSGD only touches the native library in ``step``."""
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")


class _Opt:
    def set_lr(self, lr):
        self.lr = lr


def _cfg(sfod, *opts):
    return sfod.config.setup_cfg(HOT, ["SOLVER.BASE_LR", "0.02", "SOLVER.WARMUP_ITERS", "100", "SOLVER.WARMUP_FACTOR", "0.001",
                                       "SOLVER.MAX_ITER", "1000", "SOLVER.STEPS", "(600, 800)", "SOLVER.GAMMA", "0.1"] + list(opts))


ITS = (0, 1, 99, 100, 500, 1000)      # 0, 1, WARMUP_ITERS - 1, WARMUP_ITERS, MAX_ITER // 2, MAX_ITER


def _warm(method, it):
    if it >= 100:
        return 1.0
    return 0.001 if method == "constant" else 0.001 * (1 - it / 100) + it / 100


@pytest.mark.parametrize("method", ["linear", "constant"])
def test_warmup_cosine_lr_closed_form(sfod, method):
    o = _Opt()
    cfg = _cfg(sfod, "SOLVER.LR_SCHEDULER_NAME", "WarmupCosineLR", "SOLVER.WARMUP_METHOD", method)
    sched = sfod.engine.build_lr_scheduler(cfg, o)
    assert isinstance(sched, sfod.engine.WarmupCosineLR)
    assert o.lr == sched.get_lr(0)
    for it in ITS:
        want = 0.02 * _warm(method, it) * 0.5 * (1 + math.cos(math.pi * it / 1000))
        assert abs(sched.get_lr(it) - want) < 1e-15, (it, sched.get_lr(it), want)
    assert sched.get_lr(1000) < 1e-15 and abs(sched.get_lr(500) - 0.01) < 1e-15
    for _ in range(3):          # step() walks the same closed form, state_dict round-trips
        sched.step()
    assert sched.last_epoch == 3 and o.lr == sched.get_lr(3)
    other = sfod.engine.WarmupCosineLR(_Opt(), cfg)
    other.load_state_dict(sched.state_dict())
    assert other.optimizer.lr == o.lr


@pytest.mark.parametrize("method", ["linear", "constant"])
def test_warmup_multistep_lr_with_both_warmup_methods(sfod, method):
    o = _Opt()
    sched = sfod.engine.build_lr_scheduler(_cfg(sfod, "SOLVER.WARMUP_METHOD", method), o)
    assert isinstance(sched, sfod.engine.WarmupMultiStepLR)
    for it in ITS + (599, 600, 800):
        want = 0.02 * _warm(method, it) * 0.1 ** ((it >= 600) + (it >= 800))
        assert abs(sched.get_lr(it) - want) < 1e-15, (it, sched.get_lr(it), want)


def test_scheduler_dispatch_and_unknown_names(sfod):
    with pytest.raises(ValueError, match="LR_SCHEDULER_NAME.*WarmupPolyLR"):
        sfod.engine.build_lr_scheduler(_cfg(sfod, "SOLVER.LR_SCHEDULER_NAME", "WarmupPolyLR"), _Opt())
    with pytest.raises(ValueError, match="WARMUP_METHOD.*burnin"):
        sfod.engine.build_lr_scheduler(_cfg(sfod, "SOLVER.WARMUP_METHOD", "burnin"), _Opt())


def _tree():
    """a conv with bias, a BatchNorm, a linear layer and a frozen parameter"""
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.Linear(7, 2, bias=False),
                              torch.nn.Conv2d(5, 4, 1))
    for p in net[3].parameters():
        p.requires_grad_(False)
    return net


def test_unsupported_options_raise_value_errors(sfod):
    E = sfod.engine
    on = ["SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm"]
    with pytest.raises(ValueError, match=r"NORM_TYPE = 3\.0"):
        E.build_optimizer(_cfg(sfod, *on, "SOLVER.CLIP_GRADIENTS.NORM_TYPE", "3.0"), _tree())
    with pytest.raises(ValueError, match="CLIP_TYPE = 'full_model'"):
        E.build_optimizer(_cfg(sfod, "SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model"), _tree())
    with pytest.raises(ValueError, match="NESTEROV.*MOMENTUM"):
        E.build_optimizer(_cfg(sfod, "SOLVER.NESTEROV", "True", "SOLVER.MOMENTUM", "0.0"), _tree())
    # NORM_TYPE is not read while clipping is off or by value
    assert E.build_optimizer(_cfg(sfod, "SOLVER.CLIP_GRADIENTS.NORM_TYPE", "3.0"), _tree()).clip is None
    opt = E.build_optimizer(_cfg(sfod, "SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.NORM_TYPE", "3.0"), _tree())
    assert opt.clip == {"type": "value", "value": 1.0, "norm_type": 3.0} and opt.table_driven
    opt = E.build_optimizer(_cfg(sfod, *on, "SOLVER.CLIP_GRADIENTS.NORM_TYPE", "1e999"), _tree())    # parses as the float inf
    assert opt.clip["norm_type"] == float("inf")


def test_per_parameter_hyper_parameters_follow_detectron2(sfod):
    E = sfod.engine
    # flat order: decayed (0.weight 135 -> 136 padded, 0.bias 5 -> 8, 2.weight 14 -> 16), norm (1.weight, 1.bias: 5 -> 8 each)
    opt = E.build_optimizer(_cfg(sfod), _tree())
    assert not opt.table_driven                      # every option at its default: the two-group kernels
    assert opt.hyper == [("0.weight", 0, 135, 1e-4, 1.0), ("0.bias", 136, 5, 1e-4, 1.0), ("2.weight", 144, 14, 1e-4, 1.0),
                         ("1.weight", 160, 5, 0.0, 1.0), ("1.bias", 168, 5, 0.0, 1.0)]
    assert opt.flat.n_norm_end == 176 and "3.weight" in opt.flat.offsets     # the frozen conv is laid out, not optimised
    # WEIGHT_DECAY_BIAS overrides WEIGHT_DECAY_NORM on the BatchNorm's bias; BIAS_LR_FACTOR touches biases only
    opt = E.build_optimizer(_cfg(sfod, "SOLVER.WEIGHT_DECAY_BIAS", "0.003", "SOLVER.BIAS_LR_FACTOR", "2.0",
                                 "SOLVER.WEIGHT_DECAY_NORM", "0.0005"), _tree())
    assert opt.table_driven
    assert opt.hyper == [("0.weight", 0, 135, 1e-4, 1.0), ("0.bias", 136, 5, 0.003, 2.0), ("2.weight", 144, 14, 1e-4, 1.0),
                         ("1.weight", 160, 5, 0.0005, 1.0), ("1.bias", 168, 5, 0.003, 2.0)]
    assert opt.seg_off.tolist() == [0, 136, 144, 160, 168] and opt.seg_len.tolist() == [135, 5, 14, 5, 5]
    torch.testing.assert_close(opt.seg_hp, torch.tensor([[1e-4, 1.0], [0.003, 2.0], [1e-4, 1.0], [0.0005, 1.0], [0.003, 2.0]]),
                               rtol=0, atol=0)
    # WEIGHT_DECAY_BIAS 0.0 is a value, not "unset"
    opt = E.build_optimizer(_cfg(sfod, "SOLVER.WEIGHT_DECAY_BIAS", "0.0"), _tree())
    assert [r[3] for r in opt.hyper] == [1e-4, 0.0, 1e-4, 0.0, 0.0] and opt.table_driven
    # a value that changes nothing keeps the two-group kernels; Nesterov alone does not
    assert not E.build_optimizer(_cfg(sfod, "SOLVER.WEIGHT_DECAY_BIAS", "0.0001", "SOLVER.WEIGHT_DECAY_NORM", "0.0001"), _tree()).table_driven
    assert E.build_optimizer(_cfg(sfod, "SOLVER.NESTEROV", "True"), _tree()).table_driven


def test_new_entry_points_refuse_broken_arguments_before_any_launch(sfod):
    """Host side of sfod_grad_clip_coef / sfod_sgd_ema_seg / sfod_grad_clip_ws_floats: from a valid argument list ONE
    argument is broken at a time; every such call returns SFOD_EBADARG with a message (so nothing was launched: no GPU
    is needed).  tests/test_abi.py's sanitizer fuzz covers the same entry points with random vectors."""
    import ctypes
    import threading
    lib = sfod.native.load()
    protos = sfod.native.parse_header()
    failures = []
    before = lib.sfod_last_error()      # whatever an earlier test left in this thread's record

    def body():      # sfod_last_error is per thread: the messages provoked here stay out of the other tests' thread
        try:
            _refusals(lib, protos, ctypes)
        except BaseException as e:      # noqa: BLE001 -- handed to the test's thread
            failures.append(e)
    th = threading.Thread(target=body)
    th.start()
    th.join()
    if failures:
        raise failures[0]
    assert lib.sfod_last_error() == before


def _refusals(lib, protos, ctypes):
    for name in ("sfod_grad_clip_ws_floats", "sfod_grad_clip_coef", "sfod_sgd_ema_seg"):
        assert name in protos
    assert protos["sfod_grad_clip_ws_floats"][0] is ctypes.c_int64
    q = lib.sfod_grad_clip_ws_floats
    assert q(0, 0) == 0 and q(4096, 3) == 4 and q(4100, 3) == 5 and q(35 * 10 ** 6, 300) == 8545 + 300
    assert q(-4, 3) == -1000 and q(4096, -1) == -1000 and lib.sfod_last_error()
    buf = ctypes.create_string_buffer(1 << 12)
    P = (ctypes.addressof(buf) + 63) // 64 * 64

    def refused(fn, valid, names, mutations):
        for key, val in mutations:
            a = list(valid)
            a[names.index(key)] = val
            assert fn(*a) == -1000 and lib.sfod_last_error(), (key, val)

    names = ["grad", "n", "seg_off", "seg_len", "nseg", "grad_scale", "clip_value", "norm_type", "coef", "ws", "ws_floats", "stream"]
    valid = [P, 1000, P, P, 3, 1.0, 1.0, 0, P, P, 4, None]
    refused(lib.sfod_grad_clip_coef, valid, names, [
        ("n", -4), ("n", 1001), ("n", 2 ** 41), ("nseg", -1), ("norm_type", 2), ("norm_type", -1), ("grad", None),
        ("grad", P + 4), ("seg_off", None), ("seg_len", None), ("coef", None), ("ws", None), ("ws_floats", 3), ("ws_floats", -1)])
    names = ["param", "grad", "mom", "teacher", "n", "seg_off", "nseg", "seg_hp", "clip_coef", "lr", "momentum", "grad_scale",
             "clip_type", "clip_value", "nesterov", "ema_keep", "ema_one_minus_keep", "first_step", "stream"]
    valid = [P, P, P, None, 1000, P, 3, P, P, P, 0.9, 1.0, 2, 1.0, 1, 0.9996, 0.0004, 0, None]
    refused(lib.sfod_sgd_ema_seg, valid, names, [
        ("n", -4), ("n", 1002), ("nseg", 0), ("nseg", -3), ("param", None), ("grad", None), ("mom", None), ("lr", None),
        ("seg_off", None), ("seg_hp", None), ("clip_coef", None), ("clip_type", 3), ("clip_type", -1), ("teacher", P + 8),
        ("param", P + 4)])
    a = list(valid)
    a[names.index("clip_type")], a[names.index("clip_value")] = 1, float("nan")
    assert lib.sfod_sgd_ema_seg(*a) == -1000 and lib.sfod_last_error()
