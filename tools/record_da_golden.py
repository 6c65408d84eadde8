"""Records tests/golden/da_ref.npz: the reference's DA Faster R-CNN pieces run on the closed-form inputs of
tests/helpers/da_cases.py, in float64 on the CPU.

Usage: python tools/record_da_golden.py <reference checkout> [out.npz]        (CPU only; no test reads the reference)

``daod/modeling/dann/dann.py`` is plain torch and is loaded as it is; ``daod/modeling/meta_arch/da_faster_rcnn.py`` is loaded by
file path behind oracle/ref_stub/hook.py, its ``gradient_scalar`` set to the real one of dann.py, and
``DAFasterRCNN.image_dc_loss`` / ``instance_dc_loss`` / ``consistency_loss`` are called unbound on a stub ``self`` that has the
real heads (``.double()``), the weights, and ``roi_heads.box_pooler`` served by oracle/roi_align.py (fp32 inside, whatever the
dtype around it).  The module's ``torch.FloatTensor`` label tensors are made in the heads' dtype.  ``F.dropout`` of dann.py is
replaced by recorded masks for the training-mode entries.

Stored (data only; gradients of more than 128 elements as the elements at ``da_cases.probe_indices`` plus their sum and
2-norm, see ``summarise``):
  img_head/...            DAImgHead forward on the small case's features, autograd gradients of its sum
  img_head_model/...      the same at the model case's 512 channels, gradients of sum(out * upstream)
  ins_head/{eval,train}/  DAInsHead forward on the small case's box features, gradients of its sum
  {small,model}/w{k}/l{label}/.../{img,ins,cons}/...   the three loss methods for the runs ``da_cases.SMALL_RUNS`` /
                          ``MODEL_RUNS`` (weight set, domain label, pooler; training mode with the case's masks, or eval
                          mode): value, and the gradient with respect to the features, the box features, every head
                          parameter and (model case) the box head's parameters.
  bucket/...              ``AspectRatioGroupedSemiSupDataset.__iter__`` on two streams of mixed-aspect dicts, batch sizes (2, 3):
                          the yielded ids
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LEVEL = "vgg4"
IMG_NAMES = {"conv1": "DC_img_conv1_level_" + LEVEL, "conv2": "DC_img_conv2_level_" + LEVEL}
INS_NAMES = {"fc%d" % k: "da_ins_fc%d_level_%s" % (k, LEVEL) for k in (1, 2, 3)}


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def summarise(out, key, t):
    """out[key] = t (small) or out[key + "@probe" / "@sum" / "@norm"]"""
    from helpers import da_cases as C
    t = t.detach().double().reshape(-1)
    if t.numel() <= C.PROBE:
        out[key] = t.numpy()
    else:
        out[key + "@probe"] = t[C.probe_indices(t.numel())].numpy()
        out[key + "@sum"] = np.float64(t.sum().item())
        out[key + "@norm"] = np.float64(t.norm().item())


def load_head(head, names, w):
    sd = {}
    for short, long in names.items():
        sd[long + ".weight"], sd[long + ".bias"] = w[short + ".weight"], w[short + ".bias"]
    head.load_state_dict(sd)
    return head.double()


def head_leaves(prefix, head, names):
    return {prefix + short + "." + p: getattr(getattr(head, long), p) for short, long in names.items() for p in ("weight", "bias")}


class MaskQueue:
    """stands in for ``F`` inside dann.py: ``relu`` is torch's, ``dropout`` multiplies by the next recorded mask (p = 0.5)"""

    def __init__(self):
        self.masks = []
        self.relu = torch.nn.functional.relu

    def dropout(self, x, p=0.5, training=True):
        if not training:
            return x
        assert p == 0.5
        return x * self.masks.pop(0).to(x.dtype) * 2.0


def live_order(rois):
    """rows of the live rois in the order the reference concatenates them: image by image"""
    live = torch.nonzero(rois[:, 0] >= 0).flatten()
    return live[torch.argsort(rois[live, 0], stable=True)]


def record_losses(out, prefix, ref, dann, queue, feat, box_features, rois, w_img, w_ins, weights, label, pooler, masks,
                  extra_leaves=None):
    """``box_features``: [N_ROWS, D], a leaf or a function of ``feat`` (model case); ``masks``: None = eval mode"""
    w_i, w_n, w_c = weights
    pooled, sr, aligned = pooler
    from oracle import roi_align as ora
    from helpers import da_cases as C
    order = live_order(rois)
    boxes = [rois[order][rois[order, 0] == b, 1:].double() for b in range(C.MAP[0])]

    def box_pooler(feats, box_lists):
        r = torch.cat([torch.cat([torch.full((len(bx), 1), float(b), dtype=torch.float64), bx], 1) for b, bx in enumerate(box_lists)])
        return ora.roi_align(feats[0], r, pooled, 1.0 / C.STRIDE, sr, aligned).to(feats[0].dtype)

    DC_img = load_head(dann.DAImgHead(feat.shape[1], [LEVEL]), IMG_NAMES, w_img)
    DC_ins = load_head(dann.DAInsHead(box_features.shape[1], [LEVEL]), INS_NAMES, w_ins)
    DC_img.train(masks is not None)
    DC_ins.train(masks is not None)
    stub = types.SimpleNamespace(levels=[LEVEL], DC_img=DC_img, DC_ins=DC_ins, dc_img_grl_weight=w_i, dc_ins_grl_weight=w_n,
                                 dc_consistency_weight=w_c, device=torch.device("cpu"), pooler_resolution=pooled,
                                 roi_heads=types.SimpleNamespace(box_pooler=box_pooler))
    proposals = [types.SimpleNamespace(proposal_boxes=b) for b in boxes]
    levels = torch.zeros(len(order), dtype=torch.long)
    bf = box_features[order]
    om = [[m[order] for m in pair] for pair in masks] if masks is not None else [[], []]
    cls = ref.DAFasterRCNN

    def run(which):
        if which == "img":
            return cls.image_dc_loss(stub, {LEVEL: feat}, label)
        if which == "ins":
            queue.masks = list(om[0])
            return cls.instance_dc_loss(stub, bf, levels, label)
        queue.masks = list(om[1])
        return cls.consistency_loss(stub, {LEVEL: feat}, bf, proposals, levels)

    leaves = {"feat": feat, "box_features": box_features}
    leaves.update(head_leaves("w_img/", DC_img, IMG_NAMES))
    leaves.update(head_leaves("w_ins/", DC_ins, INS_NAMES))
    leaves.update(extra_leaves or {})
    for which in ("img", "ins", "cons"):
        loss = run(which)
        assert loss.dtype == torch.float64 and not queue.masks
        out[f"{prefix}/{which}/value"] = np.float64(loss.item())
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True, retain_graph=True)
        for name, g in zip(leaves, grads):
            if g is not None:
                summarise(out, f"{prefix}/{which}/g/{name}", g)


def main():
    ref_root = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "da_ref.npz")
    from oracle.ref_stub import hook
    from helpers import da_cases as C
    from helpers import da_definitions as D
    dann = load("ref_dann", os.path.join(ref_root, "daod", "modeling", "dann", "dann.py"))
    queue = MaskQueue()
    dann.F = queue
    hook.install()
    ref = load("ref_da_faster_rcnn", os.path.join(ref_root, "daod", "modeling", "meta_arch", "da_faster_rcnn.py"))
    common = load("ref_common", os.path.join(ref_root, "daod", "data", "common.py"))
    hook.uninstall()
    ref.gradient_scalar = dann.gradient_scalar

    class TorchF64:      # the module's ``torch``: its FloatTensor label tensors in the heads' dtype
        FloatTensor = torch.DoubleTensor

        def __getattr__(self, name):
            return getattr(torch, name)
    ref.torch = TorchF64()
    out = {}

    # ---- the two heads on fixed inputs ----------------------------------------------------------------------------------
    sc = C.small_case()
    feat = sc["feat"].clone().requires_grad_(True)
    head = load_head(dann.DAImgHead(16, [LEVEL]), IMG_NAMES, sc["w_img"])
    y = head({LEVEL: feat})[LEVEL]
    out["img_head/out"] = y.detach().numpy()
    leaves = {"feat": feat, **head_leaves("w_img/", head, IMG_NAMES)}
    for name, g in zip(leaves, torch.autograd.grad(y.sum(), list(leaves.values()))):
        summarise(out, "img_head/g/" + name, g)
    mc = C.model_case()
    feat = mc["feat"].clone().requires_grad_(True)
    head = load_head(dann.DAImgHead(512, [LEVEL]), IMG_NAMES, mc["w_img"])
    y = head({LEVEL: feat})[LEVEL]
    out["img_head_model/out"] = y.detach().numpy()
    leaves = {"feat": feat, **head_leaves("w_img/", head, IMG_NAMES)}
    upstream = C.as_f32_values(C.hashed(tuple(y.shape), 77))      # a non-constant upstream gradient
    out["img_head_model/upstream"] = upstream.numpy()
    for name, g in zip(leaves, torch.autograd.grad((y * upstream).sum(), list(leaves.values()))):
        summarise(out, "img_head_model/g/" + name, g)
    for mode in ("eval", "train"):
        bf = sc["box_features"].clone().requires_grad_(True)
        head = load_head(dann.DAInsHead(32, [LEVEL]), INS_NAMES, sc["w_ins"]).train(mode == "train")
        queue.masks = list(sc["masks"][0]) if mode == "train" else []
        y = head(bf, levels=torch.zeros(C.N_ROWS, dtype=torch.long))
        out[f"ins_head/{mode}/out"] = y.detach().numpy()
        leaves = {"box_features": bf, **head_leaves("w_ins/", head, INS_NAMES)}
        for name, g in zip(leaves, torch.autograd.grad(y.sum(), list(leaves.values()))):
            summarise(out, f"ins_head/{mode}/g/" + name, g)

    # ---- the three loss methods -----------------------------------------------------------------------------------------
    for k, label, pi, mode in C.SMALL_RUNS:
        feat = sc["feat"].clone().requires_grad_(True)
        bf = sc["box_features"].clone().requires_grad_(True)
        record_losses(out, f"small/w{k}/l{label}/p{pi}/{mode}", ref, dann, queue, feat, bf, sc["rois"], sc["w_img"], sc["w_ins"],
                      C.WEIGHT_SETS[k], label, C.POOLERS[pi], sc["masks"] if mode == "train" else None)
    mc = C.model_case()
    pooler = C.POOLERS[0]
    for k, label in C.MODEL_RUNS:
        feat = mc["feat"].clone().requires_grad_(True)
        w_box = {n: v.clone().requires_grad_(True) for n, v in mc["w_box"].items()}
        rois = mc["rois"]
        live = torch.nonzero(rois[:, 0] >= 0).flatten()
        bf_live = D.box_head(feat, rois[live].double(), w_box, pooler[0], 1.0 / C.STRIDE, pooler[1], pooler[2])
        bf = torch.zeros(C.N_ROWS, bf_live.shape[1], dtype=torch.float64).index_copy(0, live, bf_live)
        record_losses(out, f"model/w{k}/l{label}/train", ref, dann, queue, feat, bf, rois, mc["w_img"], mc["w_ins"],
                      C.WEIGHT_SETS[k], label, pooler, mc["masks"], extra_leaves={"w_box/" + n: v for n, v in w_box.items()})

    # ---- the loader's two-bucket rule -------------------------------------------------------------------------------------
    for ci, (seed_a, seed_b) in enumerate(((3, 4), (5, 6))):
        wide_a = (C.hashed((60,), seed_a) >= -0.3).tolist()
        wide_b = (C.hashed((60,), seed_b) >= 0.2).tolist()
        mk = lambda wide, base: [{"width": 1200 if w else 600, "height": 600 if w else 1200, "image_id": base + i}
                                 for i, w in enumerate(wide)]
        ds = common.AspectRatioGroupedSemiSupDataset((iter(mk(wide_a, 0)), iter(mk(wide_b, 1000))), (2, 3))
        batches = list(ds)
        out[f"bucket/{ci}/wide_label"] = np.array(wide_a)
        out[f"bucket/{ci}/wide_unlabel"] = np.array(wide_b)
        out[f"bucket/{ci}/label_ids"] = np.array([[d["image_id"] for d in a] for a, _ in batches])
        out[f"bucket/{ci}/unlabel_ids"] = np.array([[d["image_id"] for d in b] for _, b in batches])
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "entries")
    for k in sorted(out):
        if k.endswith("/value"):
            print(" ", k, out[k])


if __name__ == "__main__":
    main()
