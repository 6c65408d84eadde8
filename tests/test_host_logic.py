"""Host-side mirror of the reference's config / registry / structures surface (no GPU needed)."""
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
SRC = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_source_new.yaml")


def test_config_contract_hot_yaml(sfod):
    cfg = sfod.config.setup_cfg(HOT, ["SOLVER.IMS_PER_BATCH_TARGET", "8", "INPUT.MIN_SIZE_TRAIN", "(1024,)"])
    assert cfg.TRAINER == "source_free_adaptive_teacher"
    assert cfg.MODEL.META_ARCHITECTURE == "SourceFreeAdaptiveTeacherGeneralizedRCNN"
    assert cfg.MODEL.PROPOSAL_GENERATOR.NAME == "PseudoLabRPN"
    assert cfg.MODEL.ROI_HEADS.NAME == "SourceFreeAdaptiveTeacherStandardROIHeads"
    assert cfg.SEMISUPNET.BBOX_THRESHOLD == 0.8 and cfg.SEMISUPNET.DIS_TYPE == "vgg4" and cfg.SEMISUPNET.INS_DC
    assert cfg.SOLVER.STEPS == (60000, 80000, 90000, 360000) and cfg.SOLVER.BASE_LR == 0.0025
    assert cfg.DOMAIN_CLASSIFIER.ENABLED and not cfg.DOMAIN_CLASSIFIER.IMAGE and not cfg.WEAK_STRONG_AUGMENT
    assert cfg.SOLVER.IMS_PER_BATCH_TARGET == 8 and cfg.INPUT.MIN_SIZE_TRAIN == (1024,)
    assert cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN == 12000 and cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE == 512
    assert cfg.TEST.VAL_LOSS is True and cfg.VGG.BN is True
    with pytest.raises(AttributeError):
        cfg.SEED = 1  # frozen
    with pytest.raises(KeyError):
        sfod.config.setup_cfg(HOT, ["SOLVER.NOT_A_KEY", "1"])
    with pytest.raises(ValueError):
        sfod.config.setup_cfg(HOT, ["SOLVER.BASE_LR", "abc"])
    src = sfod.config.setup_cfg(SRC)
    assert src.TRAINER == "base" and src.MODEL.META_ARCHITECTURE == "GeneralizedRCNN" and src.SOLVER.BASE_LR == 0.04


def test_registries_resolve_reference_names(sfod):
    r = sfod.registry
    for reg, names in [(r.META_ARCH_REGISTRY, ["GeneralizedRCNN", "SourceFreeAdaptiveTeacherGeneralizedRCNN"]),
                       (r.BACKBONE_REGISTRY, ["build_vgg_backbone"]),
                       (r.PROPOSAL_GENERATOR_REGISTRY, ["RPN", "PseudoLabRPN"]),
                       (r.ROI_HEADS_REGISTRY, ["StandardROIHeads", "SourceFreeAdaptiveTeacherStandardROIHeads",
                                               "AdaptiveTeacherStandardROIHeads"]),
                       (r.ROI_BOX_HEAD_REGISTRY, ["FastRCNNConvFCHead"])]:
        for n in names:
            assert reg.get(n) is not None
    with pytest.raises(KeyError):
        r.META_ARCH_REGISTRY.get("Nope")
    with pytest.raises(ValueError):
        cfg = sfod.config.setup_cfg(HOT, ["TRAINER", "da"])
        sfod.engine.get_trainer_class(cfg)


def test_model_state_dict_surface(sfod):
    cfg = sfod.config.setup_cfg(HOT)
    torch.manual_seed(0)
    model = sfod.registry.META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
    keys = list(model.state_dict().keys())
    assert sum(p.numel() for p in model.parameters()) == 47628086
    assert sum(1 for k in keys if k.startswith("backbone.")) == 91         # section 8a a1
    for k in ["backbone.vgg0.0.weight", "backbone.vgg4.7.num_batches_tracked",
              "proposal_generator.rpn_head.conv.weight", "proposal_generator.rpn_head.anchor_deltas.bias",
              "roi_heads.box_head.fc1.weight", "roi_heads.box_predictor.bbox_pred.weight",
              "DC_img.classifier.weight", "DC_ins.da_ins_fc3_level_vgg4.bias"]:
        assert k in keys, k
    assert "pixel_mean" not in keys
    assert model.backbone.size_divisibility == 0
    sh = model.backbone.output_shape()["vgg4"]
    assert (sh.channels, sh.stride) == (512, 32)
    assert model.roi_heads.box_predictor.cls_score.in_features == 1024
    assert model.roi_heads.box_pooler.min_level == model.roi_heads.box_pooler.max_level == 5
    with pytest.raises(RuntimeError):
        sfod.modeling.build_model(sfod.config.setup_cfg(HOT, ["MODEL.DEVICE", "cpu"]))  # no CPU fallback


def test_structures_and_lr_schedule(sfod):
    S = sfod.structures
    inst = S.Instances((10, 20))
    inst.gt_boxes = S.Boxes(torch.tensor([[0.0, 0.0, 5.0, 5.0], [1.0, 1.0, 30.0, 30.0]]))
    inst.gt_classes = torch.tensor([1, 2])
    assert len(inst) == 2 and inst.has("gt_boxes") and len(inst[inst.gt_classes == 2]) == 1
    b = inst.gt_boxes.clone()
    b.clip((10, 20))
    assert b.tensor[1].tolist() == [1.0, 1.0, 20.0, 10.0]
    cat = S.Instances.cat([inst, inst])
    assert len(cat) == 4
    il = S.ImageList.from_tensors([torch.zeros(3, 4, 6), torch.zeros(3, 5, 3)])
    assert tuple(il.tensor.shape) == (2, 3, 5, 6) and il.image_sizes == [(4, 6), (5, 3)]
    cfg = sfod.config.setup_cfg(HOT)

    class Opt:
        def set_lr(self, lr):
            self.lr = lr
    o = Opt()
    sched = sfod.engine.WarmupMultiStepLR(o, cfg)
    assert abs(o.lr - 0.0025 * 0.001) < 1e-15
    assert sched.milestones == [60000, 80000, 90000]      # 360000 > MAX_ITER is dropped
    assert abs(sched.get_lr(1000) - 0.0025) < 1e-15 and abs(sched.get_lr(85000) - 0.0025 * 0.01) < 1e-15
    from oracle import model as om
    for it in (0, 1, 500, 999, 1000, 59999, 60000, 95000):
        assert abs(sched.get_lr(it) - om.lr_at(it, 0.0025)) < 1e-15


def test_threshold_bbox_api_twin(sfod):
    S = sfod.structures
    inst = S.Instances((10, 10))
    inst.pred_boxes = S.Boxes(torch.rand(3, 4))
    inst.scores = torch.tensor([0.9, 0.8, 0.81])
    inst.pred_classes = torch.tensor([1, 2, 3])
    out = sfod.engine.trainer.threshold_bbox(inst, 0.8, "roih")
    assert out.gt_classes.tolist() == [1, 3]


def test_r101_config_and_resnet_module_surface(sfod):
    """BASELINE config #5: the r101 yaml selects Detectron2's build_resnet_backbone by default; module
    structure, Detectron2 state-dict keys, FREEZE_AT=2 (stem + res2 frozen, FrozenBN buffers) and the
    optimiser grouping of frozen parameters -- host logic only, no kernels."""
    import importlib
    yaml = os.path.join(ROOT, "configs", "r101_c4_cs_foggy_adaptive_teacher_source_free.yaml")
    cfg = sfod.config.setup_cfg(yaml)
    assert cfg.MODEL.BACKBONE.NAME == "build_resnet_backbone" and cfg.MODEL.RESNETS.DEPTH == 101
    assert cfg.MODEL.RESNETS.NORM == "BN" and cfg.MODEL.BACKBONE.FREEZE_AT == 2
    assert cfg.MODEL.ANCHOR_GENERATOR.SIZES == [[64, 128, 256, 512]] and cfg.MODEL.ROI_BOX_HEAD.FC_DIM == 2048
    assert cfg.SEMISUPNET.DIS_TYPE == "res4" and cfg.WEAK_STRONG_AUGMENT and not cfg.DOMAIN_CLASSIFIER.ENABLED
    assert "build_resnet_backbone" in sfod.registry.BACKBONE_REGISTRY
    rn = importlib.import_module("simple-sfod_amd.modeling.backbone_resnet")
    net = rn.ResNet(cfg)
    assert [len(getattr(net, s)) for s in ("res2", "res3", "res4")] == [3, 4, 23] and not hasattr(net, "res5")
    sh = net.output_shape()
    assert list(sh) == ["res4"] and sh["res4"].channels == 1024 and sh["res4"].stride == 16
    sd = net.state_dict()
    for k in ("stem.conv1.weight", "stem.conv1.norm.running_var", "res2.0.shortcut.norm.weight",
              "res3.0.conv1.norm.num_batches_tracked", "res4.22.conv3.norm.running_mean"):
        assert k in sd, k
    assert "stem.conv1.norm.num_batches_tracked" not in sd          # FrozenBatchNorm2d has no counter
    assert net.res3[0].conv1.stride == (2, 2) and net.res3[0].conv2.stride == (1, 1)   # STRIDE_IN_1X1
    assert all(not p.requires_grad for n, p in net.named_parameters() if n.startswith(("stem", "res2")))
    assert all(p.requires_grad for n, p in net.named_parameters() if n.startswith(("res3", "res4")))
    assert sum(p.numel() for p in net.parameters()) == 27532480
    flat = sfod.engine.FlatModelState(net)
    frozen = [n for n, (o, k, _) in flat.offsets.items() if o >= flat.n_norm_end]
    assert frozen and all(n.startswith(("stem", "res2")) for n in frozen)
    norm = [n for n, (o, k, _) in flat.offsets.items() if flat.n_decay <= o < flat.n_norm_end]
    assert norm and all(".norm." in n and n.startswith(("res3", "res4")) for n in norm)
    # the oracle restatement consumes the same state dict
    from oracle import resnet as ore
    y = ore.forward({"backbone." + k: v for k, v in sd.items()}, torch.randn(1, 3, 64, 96), depth=101, training=False)
    assert y.shape == (1, 1024, 4, 6)


def test_checkpoint_key_matching_and_loading_semantics(tmp_path):
    """simple-sfod_amd/checkpoint.py on a small CPU module: fvcore's module.-prefix stripping (only when every key
    has it), shape filter, missing / unexpected reporting, in-place loading; Detectron2's longest-suffix matching
    for ``matching_heuristics`` checkpoints; the .pkl format of convert_vgg_bn.py:156."""
    import importlib
    import pickle
    import numpy as np
    import torch
    import torch.nn as nn
    ck = importlib.import_module("simple-sfod_amd.checkpoint")

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4))
            self.head = nn.Linear(4, 2)
    torch.manual_seed(0)
    src, dst = Net(), Net()
    w_ptr = dst.backbone[0].weight.data_ptr()
    sd = {"module." + k: v.clone() for k, v in src.state_dict().items()}
    sd["module.head.weight"] = torch.zeros(3, 4)                 # wrong shape -> skipped, reported
    sd["module.extra.bias"] = torch.zeros(1)                     # unexpected
    del sd["module.backbone.1.running_var"]                      # missing
    inc = ck.load_state_into(dst, sd)
    assert inc.incorrect_shapes == [("head.weight", (3, 4), (2, 4))]
    assert inc.unexpected_keys == ["extra.bias"] and set(inc.missing_keys) == {"backbone.1.running_var", "head.weight"}
    assert torch.equal(dst.backbone[0].weight, src.backbone[0].weight) and dst.backbone[0].weight.data_ptr() == w_ptr
    assert not torch.equal(dst.head.weight, src.head.weight)
    # prefix kept when not every key carries it
    assert set(ck.strip_prefix_if_present({"module.a": 1, "b": 2}, "module.")) == {"module.a", "b"}
    # matching heuristics: checkpoint keys are suffixes of the model's
    dst2 = Net()
    heur = {"0.weight": src.backbone[0].weight.detach().numpy(), "1.running_mean": np.full(4, 7.0, dtype=np.float32),
            "head.bias": src.head.bias.detach().numpy()}
    path = tmp_path / "w.pkl"
    with open(path, "wb") as f:
        pickle.dump({"model": heur, "__author__": "torchvision", "matching_heuristics": True}, f)
    inc = ck.load_model_weights(dst2, str(path))
    assert torch.equal(dst2.backbone[0].weight, src.backbone[0].weight)
    assert torch.equal(dst2.backbone[1].running_mean, torch.full((4,), 7.0)) and torch.equal(dst2.head.bias, src.head.bias)
    assert inc.unexpected_keys == [] and "head.weight" in inc.missing_keys
    with pytest.raises(FileNotFoundError):
        ck.load_model_weights(dst2, str(tmp_path / "nope.pth"))


def test_ema_attach_raises_the_reference_error_for_a_key_the_student_lacks(sfod):
    """source_free_adaptive_teacher.py:600-601: ``Exception("{} is not found in student model")``."""
    E = sfod.engine
    student = torch.nn.Sequential(torch.nn.Linear(3, 2))
    teacher = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    fs, ft = E.FlatModelState(student), E.FlatModelState(teacher, with_grad=False)
    opt = E.solver.FusedSGD.__new__(E.solver.FusedSGD)
    opt.flat, opt.teacher, opt.ema_keep = fs, None, 0.0
    with pytest.raises(Exception, match="1.weight is not found in student model"):
        opt.attach_teacher(ft, 0.9996)
    ok = E.FlatModelState(torch.nn.Sequential(torch.nn.Linear(3, 2)), with_grad=False)
    opt.attach_teacher(ok, 0.9996)
    assert opt.teacher is ok and opt.ema_keep == 0.9996


def test_reads_checkpoints_in_the_reference_stacks_formats(sfod, tmp_path):
    """SURVEY 8f rank 2 pinned on files this package did NOT write (tests/golden/make_reference_format_checkpoints.py
    builds them by hand from the reference's key lists, manifest committed as tests/golden/ref_ckpt_manifest.json):
    (i) the ``.pkl`` layout of convert_pretrained_model/convert_vgg_bn.py:142-157 as MODEL.WEIGHTS; (ii) the ensemble
    ``.pth`` of fvcore's Checkpointer.save for DetectionTSCheckpointer(EnsembleTSModel, optimizer, scheduler)
    (source_free_adaptive_teacher.py:81-89) with a real torch.optim.SGD state dict, resumed from."""
    import importlib.util
    import json
    import pickle
    from types import SimpleNamespace
    import numpy as np
    spec = importlib.util.spec_from_file_location("mk_ref_ckpt", os.path.join(ROOT, "tests", "golden",
                                                                              "make_reference_format_checkpoints.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_ckpt_manifest.json")))
    assert man == json.loads(json.dumps(mk.manifest())), "regenerate with --manifest"
    ck = importlib.import_module("simple-sfod_amd.checkpoint")
    E = sfod.engine
    yaml = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
    cfg = sfod.config.setup_cfg(yaml, ["MODEL.ROI_BOX_HEAD.FC_DIM", "64"])          # small heads: small files

    def build(seed):
        torch.manual_seed(seed)
        return sfod.registry.META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)

    # ---- (i) convert_vgg_bn.py layout ---------------------------------------------------------------------------
    pkl_path = str(tmp_path / "vgg16_bn.pkl")
    tv, _ = mk.write_pkl(pkl_path, seed=3)
    raw = pickle.load(open(pkl_path, "rb"))
    assert list(raw.keys()) == man["pkl"]["top_level"] and raw["__author__"] == "torchvision"
    assert {k: list(v.shape) for k, v in raw["model"].items()} == man["pkl"]["model"]
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in raw["model"].values())
    model = build(0)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    inc = ck.load_model_weights(model, pkl_path, who="student")
    sd = model.state_dict()
    # every conv / BatchNorm tensor of the trunk comes from the torchvision layer of the same ordinal
    tv_convs = [k[:-7] for k in tv if k.startswith("features") and k.endswith(".weight") and tv[k].dim() == 4]
    ours = [k[:-7] for k in sd if k.startswith("backbone") and k.endswith(".weight") and sd[k].dim() == 4]
    assert len(tv_convs) == len(ours) == 13
    for a, b in zip(tv_convs, ours):
        n = int(a.split(".")[1])
        stage, idx = b.split(".")[1], int(b.split(".")[2])
        assert torch.equal(sd[b + ".weight"], tv[a + ".weight"]) and torch.equal(sd[b + ".bias"], tv[a + ".bias"])
        for s in ("weight", "bias", "running_mean", "running_var"):
            assert torch.equal(sd[f"backbone.{stage}.{idx + 1}.{s}"], tv[f"features.{n + 1}.{s}"]), (b, s)
    assert inc.unexpected_keys == [] and inc.incorrect_shapes == []
    missing = set(inc.missing_keys)
    # (num_batches_tracked: torch's BatchNorm loader fills a version-less state dict's missing counter with 0)
    assert not any(k.startswith("backbone") for k in missing)
    assert "roi_heads.box_head.fc1.weight" in missing and "proposal_generator.rpn_head.conv.weight" in missing
    assert torch.equal(sd["roi_heads.box_head.fc1.weight"], before["roi_heads.box_head.fc1.weight"])

    # ---- (ii) ensemble .pth with a torch.optim.SGD state, resumed from ----------------------------------------------
    student, teacher = build(1), build(2)
    path, moms = mk.write_ensemble_pth(str(tmp_path / "run"), student, teacher, iteration=1999, base_lr=0.0025, seed=5)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert list(raw.keys()) == man["pth"]["top_level"] and list(raw["optimizer"].keys()) == man["pth"]["optimizer"]["top_level"]
    assert all(k.startswith(tuple(man["pth"]["model_prefixes"])) for k in raw["model"])
    assert [len(g["params"]) for g in raw["optimizer"]["param_groups"]] == [len(moms) - 26, 26]   # decayed | 13 x (gamma, beta)
    s2, t2 = build(7), build(8)
    opt = E.build_optimizer(cfg, s2)
    tr = SimpleNamespace(model=s2, model_teacher=t2, optimizer=opt, scheduler=E.WarmupMultiStepLR(opt, cfg),
                         start_iter=0, iter=0)
    ck.DetectionTSCheckpointer(tr, str(tmp_path / "run")).resume_or_load("", resume=True)
    assert tr.start_iter == 2000 and tr.iter == 2000 and tr.scheduler.last_epoch == 2000
    assert abs(opt.param_groups[0]["lr"] - 0.0025) < 1e-12           # past the 1000-iteration warm-up
    for k, v in student.state_dict().items():
        assert torch.equal(s2.state_dict()[k], v), k
    for k, v in teacher.state_dict().items():
        assert torch.equal(t2.state_dict()[k], v), k
    assert len(moms) == len(opt.flat.offsets)
    for n, m in moms.items():
        o, k, shp = opt.flat.offsets[n]
        assert torch.equal(opt.mom[o:o + k].view(shp), m), n
    assert opt._steps == 1
    # Detectron2 before reduce_param_groups: one group per parameter, same index order
    sd_old = {"state": raw["optimizer"]["state"], "param_groups": []}
    order = [i for g in raw["optimizer"]["param_groups"] for i in g["params"]]
    names_by_idx = {i: n for g_t, g_o in zip(raw["optimizer"]["param_groups"], opt.torch_param_order())
                    for i, n in zip(g_t["params"], g_o)}
    walk = [n for n in opt.flat.named_order]
    renum = {n: j for j, n in enumerate(walk)}
    sd_old["state"] = {renum[names_by_idx[i]]: st for i, st in raw["optimizer"]["state"].items()}
    sd_old["param_groups"] = [{"lr": 0.001, "weight_decay": 1e-4, "params": [j]} for j in range(len(walk))]
    opt.mom.zero_()
    assert opt.load_state_dict(sd_old) == len(moms)
    for n, m in moms.items():
        o, k, shp = opt.flat.offsets[n]
        assert torch.equal(opt.mom[o:o + k].view(shp), m), n
    # Detectron2 versions whose WEIGHT_DECAY_BIAS default (= WEIGHT_DECAY) catches the norm layers' biases before the norm
    # test: merged groups [N + 13, 13] -- only the 13 BatchNorm weights form the no-decay group.  The grouping is read off
    # the checkpoint (group sizes + momentum-buffer shapes), not assumed
    g_old = opt.torch_param_order("norm_weight")
    assert [len(g) for g in g_old] == [len(moms) - 13, 13] and all(n.endswith(".weight") for n in g_old[1])
    idx, sd_b = 0, {"state": {}, "param_groups": []}
    for grp in g_old:
        sd_b["param_groups"].append({"lr": 0.0025, "weight_decay": 1e-4 if grp is g_old[0] else 0.0,
                                     "params": list(range(idx, idx + len(grp)))})
        for n in grp:
            sd_b["state"][idx] = {"momentum_buffer": moms[n].clone()}
            idx += 1
    opt.mom.zero_()
    assert opt.load_state_dict(sd_b) == len(moms)
    for n, m in moms.items():
        o, k, shp = opt.flat.offsets[n]
        assert torch.equal(opt.mom[o:o + k].view(shp), m), n
    with pytest.raises(ValueError, match="does not fit this model"):
        opt.load_state_dict({"state": {}, "param_groups": [{"lr": 0.1, "params": [0, 1, 2]}]})


def test_compute_modes_and_operand_formats(sfod):
    """SFOD.COMPUTE_DTYPE -> operand formats, host side only: every mode name resolves, the yamls select the mode their
    600x1200 gate passes in (VGG16: bf16x3; ResNet-101: f16x3), f16x3 pairs half-pair forward operands with bf16-pair
    backward operands, and the two pair formats carry distinct storage tags (a tensor of one can never be taken for the other)."""
    native = sfod.native
    assert set(native.COMPUTE_MODES) == {"fp32", "bf16", "bf16x3", "f16x3"}
    assert [native.mode_dt(n) for n in ("fp32", "bf16", "bf16x3", "f16x3")] == [native.F32, native.BF16, native.BF16X3, native.F16X3]
    assert native.mode_dt("F16X3") == native.F16X3
    with pytest.raises(ValueError):
        native.mode_dt("fp16")
    assert native.mode_dtype("bf16x3") == native.SPLIT_DTYPE and native.mode_dtype("f16x3") == native.SPLITH_DTYPE
    assert native.SPLIT_DTYPE != native.SPLITH_DTYPE
    assert torch.empty(0, dtype=native.SPLIT_DTYPE).element_size() == torch.empty(0, dtype=native.SPLITH_DTYPE).element_size() == 4
    for dtype in (torch.float32, torch.bfloat16, native.SPLIT_DTYPE, native.SPLITH_DTYPE):
        assert native.torch_dtype(native.dt_of_dtype(dtype)) == dtype
    # forward operands -> backward operands / dtype the convolutions write
    assert native.grad_dtype_of(native.SPLITH_DTYPE) == native.SPLIT_DTYPE          # gradients do not fit half's range
    assert native.grad_dtype_of(native.SPLIT_DTYPE) == native.SPLIT_DTYPE
    assert native.grad_dtype_of(torch.float32) == torch.float32 and native.grad_dtype_of(torch.bfloat16) == torch.bfloat16
    assert native.out_dtype_of(native.SPLITH_DTYPE) == native.out_dtype_of(native.SPLIT_DTYPE) == torch.float32
    assert native.is_pairs(native.SPLITH_DTYPE) and native.is_pairs(native.SPLIT_DTYPE) and not native.is_pairs(torch.float32)
    assert native.chunk_elems(native.F16X3) == native.chunk_elems(native.BF16X3) == 8
    # the header's codes are the wrapper's
    hdr = open(native.HEADER).read()
    for name, code in (("SFOD_F32", native.F32), ("SFOD_BF16", native.BF16), ("SFOD_BF16X3", native.BF16X3), ("SFOD_F16X3", native.F16X3)):
        assert f"#define {name} {code}\n" in hdr
    # which mode each yaml runs in
    cfgs = os.path.join(ROOT, "configs")
    hot = sfod.config.setup_cfg(os.path.join(cfgs, "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml"))
    r101 = sfod.config.setup_cfg(os.path.join(cfgs, "r101_c4_cs_foggy_adaptive_teacher_source_free.yaml"))
    assert hot.SFOD.COMPUTE_DTYPE == "bf16x3" and r101.SFOD.COMPUTE_DTYPE == "f16x3"
    over = sfod.config.setup_cfg(os.path.join(cfgs, "r101_c4_cs_foggy_adaptive_teacher_source_free.yaml"), ["SFOD.COMPUTE_DTYPE", "fp32"])
    assert over.SFOD.COMPUTE_DTYPE == "fp32"
    import importlib
    bench = importlib.import_module("bench")
    assert bench.PARITY_DTYPE == {"vgg": hot.SFOD.COMPUTE_DTYPE, "r101": r101.SFOD.COMPUTE_DTYPE}


def test_split_precision_definitions_and_their_own_error():
    """oracle/split_precision.py (what the pair modes are defined to compute) on the CPU: the pairs are exact splits, the
    weight scale is the packers' power of two, and the definitions sit where DESIGN.md 1a says they do relative to the exact
    product -- bf16 pairs ~4.5e-6 (16-bit operands), half pairs ~8e-8 (22-bit operands under the weight scale), and half pairs
    WITHOUT the scale 4x worse on kaiming-sized weights (lo falls into half's subnormals)."""
    from oracle import split_precision as sp
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(128, 1024, generator=g)) + 0.01 * torch.randn(128, 1024, generator=g)
    w = torch.randn(64, 1024, generator=g) * (2.0 / 1024) ** 0.5
    for fmt, bits in (("bf16", 16), ("f16", 22)):
        hi, lo = sp.split_pairs(x, fmt)
        assert ((hi + lo - x.double()).abs() <= x.double().abs() * 2.0 ** -bits + 2.0 ** -25).all()
        assert torch.equal(hi.float().double(), hi) and torch.equal(lo.float().double(), lo)      # 16-bit values: exact in fp32
    s = sp.weight_scale(w)
    assert math.log2(s) == int(math.log2(s)) and 2.0 ** 13 <= float(w.abs().max()) * s < 2.0 ** 14
    assert sp.weight_scale(torch.zeros(4, 4)) == 1.0
    exact = x.double() @ w.double().t()
    err = lambda y: ((y - exact).norm() / exact.norm()).item()
    e_bf, e_h = err(sp.linear(x, w, "bf16")), err(sp.linear(x, w, "f16"))
    xh, xl = sp.split_pairs(x, "f16")
    wh, wl = sp.split_pairs(w, "f16")                     # unscaled weights
    e_h_unscaled = err(xh @ wh.t() + xh @ wl.t() + xl @ wh.t())
    assert 2e-6 < e_bf < 8e-6 and e_h < 2e-7 and e_h < e_bf / 20, (e_bf, e_h)
    assert e_h_unscaled > 2.5 * e_h, (e_h_unscaled, e_h)
    # every mode through the generic helpers: linear_mode of the pair modes IS linear(); the plain modes are exact products
    for mode, fmt in sp.PAIR_FORMAT.items():
        assert torch.equal(sp.linear_mode(x, w, mode), sp.linear(x, w, fmt))
    assert torch.equal(sp.linear_mode(x, w, "fp32"), exact)
    assert torch.equal(sp.linear_mode(x, w, "bf16"), x.bfloat16().double() @ w.bfloat16().double().t())
    # the convolution definitions equal linear() on the unfolded (im2col) operands, for every mode, stride and padding
    xc = torch.randn(2, 24, 9, 11, generator=g) + 0.3
    wc = torch.randn(40, 24, 3, 3, generator=g) / 15
    for mode in sp.MODES:
        for pad, stride in ((1, 1), (0, 1), (3, 2)):
            y = sp.conv2d(xc, wc, mode, padding=pad, stride=stride)
            cols = torch.nn.functional.unfold(xc, 3, padding=pad, stride=stride)           # [B, Cin * 9, L]
            flat = cols.transpose(1, 2).reshape(-1, 24 * 9)
            ref = sp.linear_mode(flat, wc.reshape(40, -1), mode).reshape(2, -1, 40).transpose(1, 2).reshape(y.shape)
            torch.testing.assert_close(y, ref, rtol=1e-13, atol=1e-13)
            mag = sp.magnitude(xc, wc, padding=pad, stride=stride)
            assert (mag * (1 + 2.0 ** -7) >= y.abs()).all()          # (bf16 operands: within their own rounding)
        # the weight gradient: d/dw of <conv2d(x, w), dy> summed over the same split pairs (f16x3: bf16 pairs)
        dy = torch.randn(2, 40, 9, 11, generator=g) * 1e-3
        dw = sp.conv2d_wgrad(xc, dy, wc.shape, mode)
        cols = torch.nn.functional.unfold(xc, 3, padding=1).transpose(1, 2).reshape(-1, 24 * 9)
        dyr = dy.permute(0, 2, 3, 1).reshape(-1, 40)
        ref = sp.linear_mode(dyr.t().contiguous(), cols.t().contiguous(), "bf16x3" if mode == "f16x3" else mode)
        torch.testing.assert_close(dw.reshape(40, -1), ref, rtol=1e-12, atol=1e-18)
        assert (sp.magnitude_wgrad(xc, dy, wc.shape) * (1 + 2.0 ** -7) >= dw.abs()).all()
    # the data gradient through rot180 weights is the adjoint of the forward convolution
    dy = torch.randn(2, 40, 9, 11, generator=g, dtype=torch.float64)
    dx = torch.nn.functional.conv2d(dy, sp.rot180(wc.double()), padding=1)
    xr = torch.randn(2, 24, 9, 11, generator=g, dtype=torch.float64)
    lhs = (torch.nn.functional.conv2d(xr, wc.double(), padding=1) * dy).sum()
    assert abs(float(lhs - (xr * dx).sum())) < 1e-9 * float(lhs.abs() + 1)
    # f16x3 forward weights stay under their scale: the definition divides it back out exactly
    hs, s = sp.terms(xc, wc, "f16x3", scale_b=True)
    assert s == sp.weight_scale(wc) and 2.0 ** 13 <= float((hs[0][1] + hs[1][1]).abs().max()) < 2.0 ** 14 + 1


def test_teacher_pass_defers_batchnorm_only_where_it_pays(sfod, monkeypatch):
    """backbone_vgg._defer_bn (SFOD.FUSE_BN_INPUT): a layer's BatchNorm + ReLU is left to the next convolution only in a
    forward-only train-mode pass, only for layers nobody else reads (no pooling, not a stage output), only where the library
    serves the consumer's shape and only where the pre-BatchNorm tensor is larger than the Infinity Cache."""
    yaml = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "configs",
                        "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
    cfg = sfod.config.setup_cfg(yaml, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", "bf16x3"])
    bb = sfod.modeling.backbone_vgg.build_vgg_backbone(cfg, None).train()
    assert bb.fuse_bn_input and bb.fuse_bn_input_min_bytes == 256 << 20
    asked = []
    monkeypatch.setattr(sfod.native, "conv_fwd_bnin_supported", lambda y, w, cout: asked.append((tuple(y.shape), cout)) or True)
    names = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3",
             "conv5_1", "conv5_2", "conv5_3"]
    assert len(bb._plan) == len(names)
    fwd_w = [None] * len(names)

    def deferred(batch, save=False, training=True):
        out = []
        h, w = 600, 1200
        for li, (conv, _, pool, _) in enumerate(bb._plan):
            y = torch.empty(batch, h, w, conv.out_channels, device="meta")
            if bb._defer_bn(li, y, fwd_w, save, training):
                out.append(names[li])
            if pool:
                h, w = h // 2, w // 2
        return out

    # a teacher batch of 8 frames: conv2_1 (737 MB), conv3_1 / conv3_2 (368 MB); conv1_1 is 2.9 GB but the first layer has its
    # own fused form upstream of this decision; conv4_x (184 MB) fits the cache
    assert deferred(8) == ["conv1_1", "conv2_1", "conv3_1", "conv3_2"]
    assert deferred(1) == []                                # one frame: every tensor fits the cache (conv1_1: 184 MB)
    assert deferred(8, save=True) == [] and deferred(8, training=False) == []
    bb.fuse_bn_input_min_bytes = 0                          # every non-pooled, non-stage-end layer the library serves
    assert deferred(8) == ["conv1_1", "conv2_1", "conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv5_1", "conv5_2"]
    bb.fuse_bn_input = False
    assert deferred(8) == []
    monkeypatch.setattr(sfod.native, "conv_fwd_bnin_supported", lambda y, w, cout: False)
    bb.fuse_bn_input = True
    assert deferred(8) == []


def test_offchain_helpers_are_plain_calls_without_a_gpu(sfod):
    """modeling/offchain.py on CPU tensors: ``run`` is the call itself, ``join`` nothing, a loss-gradient mark is neither made
    nor taken -- the heads' backward code paths are the single-stream ones (what the CPU-side oracle comparisons of the
    modules' host logic rely on)."""
    oc = sfod.modeling.offchain
    off = oc.OffChain(False)
    assert off.side is None
    seen = []
    assert off.run(lambda: (seen.append(1), 7)[1], torch.zeros(2)) == 7 and seen == [1]
    assert off.run(lambda: (seen.append(2), 8)[1], None, torch.zeros(2), after=None) == 8 and seen == [1, 2]
    assert off.wait() is None
    off.join(torch.zeros(1), None)
    assert seen == [1, 2]
    assert not oc.heads_on(torch.zeros(1))
    g = torch.arange(4.0)
    oc.mark_loss_grads_ready(g)
    assert oc.take_loss_grads_ready(g[1]) is None


def test_pooler_resolution_beyond_the_backward_kernel_is_refused_before_the_losses(sfod):
    """config.py's POOLER_RESOLUTION default is Detectron2's 14; the ROIAlign backward serves <= 8.  A TRAINING forward with
    gradients enabled says so at once (advisor, round 5: it used to surface as EBADARG in the first backward); forward-only
    passes (no_grad: the teacher, evaluation, Detectron2's own 14 x 14 unit-test size) are not affected."""
    import types
    import pytest
    import torch
    RH = sfod.modeling.roi_heads.StandardROIHeads
    stub = types.SimpleNamespace(in_features=["vgg4"], training=True, pooled=14)
    feats = {"vgg4": torch.zeros(1, 8, 4, 4)}
    props = sfod.modeling.batched.BatchedProposals(torch.zeros(1, 1, 4), torch.zeros(1, 1), torch.ones(1, dtype=torch.int32), [(64, 64)])
    with pytest.raises(ValueError, match="POOLER_RESOLUTION 14"):
        RH.forward(stub, None, feats, props, targets=object(), compute_loss=True)
    stub.pooled = 7          # the named yamls' value passes this point (and then needs real targets)
    with pytest.raises((AttributeError, TypeError, AssertionError)):
        RH.forward(stub, None, feats, props, targets=object(), compute_loss=True)


def test_periodic_writer_reports_the_median_of_the_last_twenty_values_like_d2s_json_writer(sfod):
    """d2 ``JSONWriter`` writes ``storage.latest_with_smoothing_hint(20)``: a scalar put with the (default) smoothing hint is
    reported as numpy's median of its last 20 values, one put with ``smoothing_hint=False`` (d2's EvalHook / LR hook) as its
    last value; records are stamped with the iteration the scalars were put in.  ``flush()`` without ``smooth`` (bench.py,
    the per-step readers of the tests) stays the last value."""
    import numpy as np
    st = sfod.engine.trainer.EventStorage()
    vals = [3.0, 9.0, 1.0, 7.0, 5.0, 11.0]
    for i, v in enumerate(vals):
        st.iter = i
        st.put_scalar("loss_a", torch.tensor(v))                  # device-style scalar
        st.put_scalar("host_b", v * 2)                             # plain float
        st.put_scalars(smoothing_hint=False, **{"bbox/AP50": v})
    rec = st.flush(smooth=True)
    assert rec["iteration"] == 5
    assert rec["loss_a"] == float(np.median(vals)) == 6.0 and rec["host_b"] == 12.0 and rec["bbox/AP50"] == 11.0
    # the window outlives a flush (d2's HistoryBuffer does) and holds the last 20 values only
    more = [float(x) for x in range(100, 125)]
    for v in more:
        st.put_scalar("loss_a", torch.tensor(v))
    assert st.flush(smooth=True)["loss_a"] == float(np.median(more[-20:]))
    st.put_scalar("loss_a", torch.tensor(-1.0))
    assert st.flush()["loss_a"] == -1.0                            # unsmoothed reader: the last value
    # a key switched to "no hint" forgets its window
    st.put_scalar("loss_a", 4.0, smoothing_hint=False)
    assert st.flush(smooth=True)["loss_a"] == 4.0
