"""Conditional DA Faster R-CNN (``CDAFasterRCNN`` / ``CDAStandardROIHeads`` behind TRAINER "da") without a device: registries,
the option matrix of modeling/da_options.py, state-dict names, the definitions of tests/helpers/cda_definitions.py against the
reference's recorded values (tests/golden/cda_ref.npz, written by tools/record_cda_golden.py from the reference's own code),
and the algebra of the one-fc1 execution the device path uses.
"""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import cda_cases as C
from helpers import cda_definitions as CD
from helpers import da_definitions as D

CONFIGS = os.path.join(os.path.dirname(GOLDEN), "..", "configs")
CDA_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_cda.yaml")
DA_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_da.yaml")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "cda_ref.npz"), allow_pickle=False)


def cfg_of(sfod, *opts, yaml=CDA_YAML):
    return sfod.config.setup_cfg(yaml, ["OUTPUT_DIR", ""] + list(opts))


def options():
    return import_module("simple-sfod_amd.modeling.da_options")


# ---- registries, options, state dict ---------------------------------------------------------------------------------------------
def test_registries_resolve_the_cda_names(sfod):
    r = sfod.registry
    m = sfod.modeling.cda_faster_rcnn
    assert r.META_ARCH_REGISTRY.get("CDAFasterRCNN") is m.CDAFasterRCNN
    assert r.ROI_HEADS_REGISTRY.get("CDAStandardROIHeads") is sfod.modeling.roi_heads.CDAStandardROIHeads
    assert issubclass(m.CDAFasterRCNN, sfod.modeling.da_faster_rcnn.DAFasterRCNN)
    assert issubclass(sfod.modeling.roi_heads.CDAStandardROIHeads, sfod.modeling.roi_heads.DAStandardROIHeads)


def test_the_cda_yaml_is_the_da_yaml_with_two_names_and_the_entropy_switch(sfod):
    a, b = cfg_of(sfod), cfg_of(sfod, yaml=DA_YAML)
    assert (a.MODEL.META_ARCHITECTURE, a.MODEL.ROI_HEADS.NAME) == ("CDAFasterRCNN", "CDAStandardROIHeads")
    assert a.DA_FASTER.ENTROPY_CONDITIONING is True and a.TRAINER == "da"
    a.defrost()
    a.MODEL.META_ARCHITECTURE, a.MODEL.ROI_HEADS.NAME = b.MODEL.META_ARCHITECTURE, b.MODEL.ROI_HEADS.NAME
    a.DA_FASTER.ENTROPY_CONDITIONING = False
    assert a == b


@pytest.mark.parametrize("entropy", [True, False])
def test_both_architectures_pass_under_the_da_trainer(sfod, entropy):
    O = options()
    cfg = cfg_of(sfod, "DA_FASTER.ENTROPY_CONDITIONING", str(entropy))
    o = O.validate_da_trainer_cfg(cfg)
    assert o.conditional is True and o.entropy_conditioning is entropy
    assert (o.level, o.img_weight, o.ins_weight, o.consistency_weight) == ("vgg4", 0.01, 0.1, 0.1)
    assert sfod.engine.get_trainer_class(cfg) is sfod.engine.DATrainer
    o = O.validate_da_trainer_cfg(cfg_of(sfod, yaml=DA_YAML))
    assert o.conditional is False and o.entropy_conditioning is False


@pytest.mark.parametrize("yaml, opts, key", [
    (CDA_YAML, ["MODEL.META_ARCHITECTURE", "GeneralizedRCNN"], "MODEL.META_ARCHITECTURE"),
    (CDA_YAML, ["MODEL.ROI_HEADS.NAME", "DAStandardROIHeads"], "MODEL.ROI_HEADS.NAME"),             # mismatched pairs
    (CDA_YAML, ["MODEL.ROI_HEADS.NAME", "StandardROIHeads"], "MODEL.ROI_HEADS.NAME"),
    (DA_YAML, ["MODEL.ROI_HEADS.NAME", "CDAStandardROIHeads"], "MODEL.ROI_HEADS.NAME"),
    (DA_YAML, ["DA_FASTER.ENTROPY_CONDITIONING", "True"], "DA_FASTER.ENTROPY_CONDITIONING"),       # only CDA reads it
    (CDA_YAML, ["DA_FASTER.LEVELS", "['vgg3', 'vgg4']"], "DA_FASTER.LEVELS"),
    (CDA_YAML, ["DA_FASTER.LEVELS", "['vgg3']"], "DA_FASTER.LEVELS"),
    (CDA_YAML, ["DA_FASTER.DC_IMG_GRL_WEIGHT", "-0.1"], "DA_FASTER.DC_IMG_GRL_WEIGHT"),
    (CDA_YAML, ["DA_FASTER.DC_INS_GRL_WEIGHT", "1e999"], "DA_FASTER.DC_INS_GRL_WEIGHT"),
    (CDA_YAML, ["DA_FASTER.DC_CONSISTENCY_WEIGHT", "-1e999"], "DA_FASTER.DC_CONSISTENCY_WEIGHT"),
    (CDA_YAML, ["MODEL.ROI_BOX_HEAD.NUM_FC", "0", "MODEL.ROI_BOX_HEAD.NUM_CONV", "1"], "MODEL.ROI_BOX_HEAD.NUM_FC"),
])
def test_validation_names_the_key(sfod, yaml, opts, key):
    cfg = cfg_of(sfod, *opts, yaml=yaml)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        options().validate_da_trainer_cfg(cfg)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        sfod.engine.get_trainer_class(cfg)


def test_entropy_conditioning_must_be_a_bool(sfod):
    cfg = cfg_of(sfod)
    cfg.defrost()
    for bad in (1, "True", None):
        cfg.DA_FASTER.ENTROPY_CONDITIONING = bad
        with pytest.raises(ValueError, match=r"DA_FASTER\.ENTROPY_CONDITIONING"):
            options().da_options(cfg)


def test_state_dict_keys_and_shapes_are_the_references(sfod):
    torch.manual_seed(0)
    cfg = cfg_of(sfod)
    model = sfod.registry.META_ARCH_REGISTRY.get("CDAFasterRCNN")(cfg)
    sd = model.state_dict()
    want = {f"DC_img.DC_img_conv{k}_level_vgg4.{p}" for k in (1, 2) for p in ("weight", "bias")} | \
           {f"DC_ins.da_ins_fc{k}_level_vgg4.{p}" for k in (1, 2, 3) for p in ("weight", "bias")}
    assert {k for k in sd if k.startswith("DC_")} == want
    assert not any("multilinear_map" in k for k in sd) and isinstance(model.multilinear_map, torch.nn.Module)
    K, Dm = cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.MODEL.ROI_BOX_HEAD.FC_DIM
    assert tuple(sd["DC_ins.da_ins_fc1_level_vgg4.weight"].shape) == (1024, Dm * (K + 1)) == (1024, 9216)
    assert tuple(sd["DC_ins.da_ins_fc2_level_vgg4.weight"].shape) == (1024, 1024)
    assert tuple(sd["DC_ins.da_ins_fc3_level_vgg4.weight"].shape) == (1, 1024)
    assert tuple(sd["DC_img.DC_img_conv1_level_vgg4.weight"].shape) == (512, 512, 1, 1)
    assert model.entropy_conditioning is True and model.da.conditional
    # the same detector keys as the DA architecture: only DC_ins' first layer differs in shape
    da = sfod.registry.META_ARCH_REGISTRY.get("DAFasterRCNN")(cfg_of(sfod, yaml=DA_YAML)).state_dict()
    assert set(da) == set(sd)
    assert {k for k in sd if sd[k].shape != da[k].shape} == {"DC_ins.da_ins_fc1_level_vgg4.weight"}


# ---- the definitions against the recorded reference values -------------------------------------------------------------------
def check_recorded(fx, key, t, rel=1e-12):
    """tests/test_da_host.py's check of a recorded tensor (whole, or probes + sum + norm)"""
    t = t.detach().double().reshape(-1)
    if key in fx.files:
        ref = torch.from_numpy(fx[key]).reshape(-1)
        assert ref.numel() == t.numel(), key
        scale = max(float(ref.abs().max()), 1e-300)
        assert float((t - ref).abs().max()) <= rel * scale, (key, float((t - ref).abs().max()), scale)
        return
    ref = torch.from_numpy(fx[key + "@probe"])
    norm = float(fx[key + "@norm"])
    got = t[C.probe_indices(t.numel())]
    assert float((got - ref).abs().max()) <= rel * max(float(ref.abs().max()), norm / t.numel() ** 0.5), key
    assert abs(float(t.norm()) - norm) <= 1e-10 * norm, key
    assert abs(float(t.sum()) - float(fx[key + "@sum"])) <= 1e-9 * max(norm, 1e-300), key


def leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize("run", C.RUNS, ids=lambda r: C.run_name(*r).replace("/", "-"))
def test_loss_definitions_equal_the_recorded_reference(fx, run):
    k, label, ent, mode = run
    sc = C.small_case()
    assert tuple(sc["scores"].shape) == (C.N_ROWS, 9) and tuple(sc["w_ins"]["fc1.weight"].shape) == (1024, 288)
    assert torch.isnan(sc["scores"][list(C.PAD_ROWS)]).all()
    feat, bf = leaf(sc["feat"]), leaf(sc["box_features"])
    w_img, w_ins = {n: leaf(v) for n, v in sc["w_img"].items()}, {n: leaf(v) for n, v in sc["w_ins"].items()}
    res = CD.evaluate_losses(feat, bf, sc["scores"], sc["rois"], w_img, w_ins, C.WEIGHT_SETS[k], label, C.POOLERS[0], ent,
                             sc["masks"] if mode == "train" else None, pool="oracle")
    prefix = "small/" + C.run_name(*run)
    seen = 0
    for which, (value, grads) in res.items():
        ref = float(fx[f"{prefix}/{which}/value"])
        assert abs(value.item() - ref) <= 1e-12 * abs(ref), (which, value.item(), ref)
        recorded = {f.split("/g/", 1)[1].split("@")[0] for f in fx.files if f.startswith(f"{prefix}/{which}/g/")}
        assert recorded == set(grads), (which, recorded ^ set(grads))
        for n, g in grads.items():
            assert torch.isfinite(g).all(), (which, n)
            check_recorded(fx, f"{prefix}/{which}/g/{n}", g)
            seen += 1
    assert seen >= 20


def test_entropy_weights_change_the_instance_loss_and_nothing_else(fx):
    for k, label in ((0, 0), (1, 1)):
        for mode in ("train", "eval"):
            a, b = "small/" + C.run_name(k, label, False, mode), "small/" + C.run_name(k, label, True, mode)
            assert float(fx[a + "/ins/value"]) != float(fx[b + "/ins/value"])
            assert float(fx[a + "/cons/value"]) == float(fx[b + "/cons/value"])
            assert float(fx[a + "/img/value"]) == float(fx[b + "/img/value"])


def test_pieces_of_the_definition():
    """index order of the conditioned feature, the entropy weight's range and its extremes, the weighted mean's normalisation"""
    f = C.as_f32_values(C.hashed((5, 8), 3))
    p = CD.condition(C.scores(5, 3, 9).double())
    x = CD.conditioned(f, p)
    assert tuple(x.shape) == (5, 24) and x[2, 1 * 8 + 5].item() == (p[2, 1] * f[2, 5]).item()
    assert torch.equal(x, torch.bmm(p.unsqueeze(2), f.unsqueeze(1)).view(5, -1))
    w = CD.entropy_weight(p)
    assert (w > 1).all() and (w <= 2 + 1e-4).all()
    assert abs(w[0].item() - (1 + 1.0 / 3 * (1 + 3e-5))) < 1e-4          # uniform over 3 classes: H ~ ln 3
    assert abs(w[1].item() - 2.0) < 1e-4                                  # one-hot: H ~ 0
    z = C.as_f32_values(C.hashed((5,), 4, 3.0))
    assert abs(CD.weighted_bce(z, 1.0, torch.full((5,), 3.0, dtype=torch.float64))[0].item() - D.bce(z, 1.0)[0].item()) < 1e-15
    dx = C.hashed((5, 24), 5)
    assert torch.allclose(CD.contraction(dx, p), sum(p[:, c: c + 1] * dx[:, c * 8: (c + 1) * 8] for c in range(3)), rtol=0, atol=1e-15)
    none = torch.zeros(5, dtype=torch.bool)
    assert CD.weighted_bce(z, 1.0, w, none)[0].item() == 0.0


# ---- the one-fc1 execution -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("entropy", [False, True])
def test_one_fc1_evaluation_equals_two_in_float64(mode, entropy):
    """What the device path relies on: with fc1 + ReLU shared, its parameters taking d1_ins + d1_cons and its input
    -w_n d1_ins + w_c w_n d1_cons, every gradient of (instance loss + consistency loss) equals autograd through the module's
    two separate evaluations, to 1e-12 relative."""
    sc = C.small_case()
    w_i, w_n, w_c = C.WEIGHT_SETS[1]
    label, pooler = 1, C.POOLERS[0]
    rois = sc["rois"]
    live = rois[:, 0] >= 0
    masks = [[m[live] for m in pair] for pair in sc["masks"]] if mode == "train" else None
    scores = sc["scores"][live].double()
    feat = sc["feat"]
    # two evaluations, by autograd
    bf, w_ins = leaf(sc["box_features"][live]), {n: leaf(v) for n, v in sc["w_ins"].items()}
    l_ins = CD.conditional_instance_dc_loss(bf, scores, w_ins, label, w_n, entropy, masks[0] if masks else None)
    l_cons = CD.conditional_consistency_loss(feat, bf, scores, rois[live].double(), sc["w_img"], w_ins, w_i, w_n, w_c, pooler[0],
                                             1.0 / C.STRIDE, pooler[1], pooler[2], masks[1] if masks else None)
    names = ["box_features"] + list(w_ins)
    two = dict(zip(names, torch.autograd.grad(l_ins + l_cons, [bf] + list(w_ins.values()))))
    # one fc1 evaluation, backward by hand from the two logit gradients
    p = CD.condition(scores)
    x = CD.conditioned(sc["box_features"][live], p)
    z_img = D.img_head(feat, sc["w_img"])[:, 0]

    def dz_fn(z_ins, z_cons):
        zi, zc = leaf(z_ins), leaf(z_cons)
        li = CD.weighted_bce(zi, label, CD.entropy_weight(p))[0] if entropy else D.bce(zi, label)[0]
        lc = D.consistency(z_img, zc, rois[live].double(), pooler[0], 1.0 / C.STRIDE, pooler[1], pooler[2])[0]
        assert abs(li.item() - l_ins.item()) <= 1e-12 * abs(l_ins.item()) and abs(lc.item() - l_cons.item()) <= 1e-12 * abs(l_cons.item())
        return torch.autograd.grad(li, zi)[0], torch.autograd.grad(lc, zc)[0]

    _, _, dx, g = CD.one_fc1_form(x, sc["w_ins"], dz_fn, w_n, w_c, masks)
    one = {"box_features": CD.contraction(dx, p), **g}
    for n in names:
        scale = float(two[n].abs().max())
        assert scale > 0, n
        err = float((one[n] - two[n]).abs().max())
        assert err <= 1e-12 * scale, (n, err, scale)
