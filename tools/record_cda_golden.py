"""Records tests/golden/cda_ref.npz: the reference's conditional DA Faster R-CNN losses run on the closed-form inputs of
tests/helpers/cda_cases.py, in float64 on the CPU.

Usage: python tools/record_cda_golden.py <reference checkout> [out.npz]        (CPU only; no test reads the reference)

Like tools/record_da_golden.py (whose helpers this imports): ``daod/modeling/dann/dann.py`` and ``daod/modeling/utils.py`` are
plain torch and are loaded as they are; ``daod/modeling/meta_arch/cda_faster_rcnn.py`` is loaded by file path behind
oracle/ref_stub/hook.py, its ``gradient_scalar`` and ``entropy`` set to the real ones, and
``CDAFasterRCNN.image_dc_loss`` / ``conditional_instance_dc_loss`` / ``conditional_consistency_loss`` are called unbound on a
stub ``self`` that has the real heads (``.double()``), the module's own ``MultiLinearMap``, the weights, the entropy switch
and ``roi_heads.box_pooler`` served by oracle/roi_align.py.  ``F.dropout`` of dann.py is replaced by recorded masks for the
training-mode entries.  The reference sees the live rows only, image by image, as its ROI heads hand them over.

Stored (data only; gradients of more than 128 elements as the elements at ``da_cases.probe_indices`` plus their sum and
2-norm, ``record_da_golden.summarise``), for case in small / model and every run of ``cda_cases.RUNS`` (weight set, domain
label, entropy conditioning, train with the case's masks / eval), pooler 0:
  {case}/w{k}/l{label}/e{0,1}/{train,eval}/{img,ins,cons}/value and .../g/<leaf>: the gradient with respect to the features,
  the box features, every head parameter and (model case) the box head's parameters.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_da_golden as R      # noqa: E402

LEVEL = R.LEVEL


def record_losses(out, prefix, ref, dann, queue, feat, box_features, scores, rois, w_img, w_ins, weights, label, pooler, entropy,
                  masks, extra_leaves=None):
    """``box_features``: [N_ROWS, D], a leaf or a function of ``feat`` (model case); ``masks``: None = eval mode"""
    w_i, w_n, w_c = weights
    pooled, sr, aligned = pooler
    from oracle import roi_align as ora
    from helpers import cda_cases as C
    order = R.live_order(rois)
    boxes = [rois[order][rois[order, 0] == b, 1:].double() for b in range(C.MAP[0])]

    def box_pooler(feats, box_lists):
        r = torch.cat([torch.cat([torch.full((len(bx), 1), float(b), dtype=torch.float64), bx], 1) for b, bx in enumerate(box_lists)])
        return ora.roi_align(feats[0], r, pooled, 1.0 / C.STRIDE, sr, aligned).to(feats[0].dtype)

    DC_img = R.load_head(dann.DAImgHead(feat.shape[1], [LEVEL]), R.IMG_NAMES, w_img)
    DC_ins = R.load_head(dann.DAInsHead(box_features.shape[1] * scores.shape[1], [LEVEL]), R.INS_NAMES, w_ins)
    DC_img.train(masks is not None)
    DC_ins.train(masks is not None)
    stub = types.SimpleNamespace(levels=[LEVEL], DC_img=DC_img, DC_ins=DC_ins, dc_img_grl_weight=w_i, dc_ins_grl_weight=w_n,
                                 dc_consistency_weight=w_c, device=torch.device("cpu"), pooler_resolution=pooled,
                                 entropy_conditioning=entropy, multilinear_map=ref.MultiLinearMap(),
                                 roi_heads=types.SimpleNamespace(box_pooler=box_pooler))
    proposals = [types.SimpleNamespace(proposal_boxes=b) for b in boxes]
    levels = torch.zeros(len(order), dtype=torch.long)
    bf = box_features[order]
    sc = scores[order].double()
    assert torch.isfinite(sc).all()
    om = [[m[order] for m in pair] for pair in masks] if masks is not None else [[], []]
    cls = ref.CDAFasterRCNN

    def run(which):
        if which == "img":
            return cls.image_dc_loss(stub, {LEVEL: feat}, label)
        if which == "ins":
            queue.masks = list(om[0])
            return cls.conditional_instance_dc_loss(stub, bf, sc, levels, label)
        queue.masks = list(om[1])
        return cls.conditional_consistency_loss(stub, {LEVEL: feat}, bf, sc, proposals, levels)

    leaves = {"feat": feat, "box_features": box_features}
    leaves.update(R.head_leaves("w_img/", DC_img, R.IMG_NAMES))
    leaves.update(R.head_leaves("w_ins/", DC_ins, R.INS_NAMES))
    leaves.update(extra_leaves or {})
    for which in ("img", "ins", "cons"):
        loss = run(which)
        assert loss.dtype == torch.float64 and not queue.masks
        out[f"{prefix}/{which}/value"] = np.float64(loss.item())
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True, retain_graph=True)
        for name, g in zip(leaves, grads):
            if g is not None:
                R.summarise(out, f"{prefix}/{which}/g/{name}", g)


def main():
    ref_root = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "cda_ref.npz")
    from oracle.ref_stub import hook
    from helpers import cda_cases as C
    from helpers import da_definitions as D
    dann = R.load("ref_dann", os.path.join(ref_root, "daod", "modeling", "dann", "dann.py"))
    utils = R.load("ref_utils", os.path.join(ref_root, "daod", "modeling", "utils.py"))
    queue = R.MaskQueue()
    dann.F = queue
    hook.install()
    ref = R.load("ref_cda_faster_rcnn", os.path.join(ref_root, "daod", "modeling", "meta_arch", "cda_faster_rcnn.py"))
    hook.uninstall()
    ref.gradient_scalar = dann.gradient_scalar
    ref.entropy = utils.entropy

    class TorchF64:      # the module's ``torch``: its FloatTensor label tensors in the heads' dtype
        FloatTensor = torch.DoubleTensor

        def __getattr__(self, name):
            return getattr(torch, name)
    ref.torch = TorchF64()
    out = {}
    pooler = C.POOLERS[0]
    sc = C.small_case()
    for k, label, ent, mode in C.RUNS:
        feat = sc["feat"].clone().requires_grad_(True)
        bf = sc["box_features"].clone().requires_grad_(True)
        record_losses(out, "small/" + C.run_name(k, label, ent, mode), ref, dann, queue, feat, bf, sc["scores"], sc["rois"],
                      sc["w_img"], sc["w_ins"], C.WEIGHT_SETS[k], label, pooler, ent, sc["masks"] if mode == "train" else None)
    mc = C.model_case()
    for k, label, ent, mode in C.RUNS:
        feat = mc["feat"].clone().requires_grad_(True)
        w_box = {n: v.clone().requires_grad_(True) for n, v in mc["w_box"].items()}
        rois = mc["rois"]
        live = torch.nonzero(rois[:, 0] >= 0).flatten()
        bf_live = D.box_head(feat, rois[live].double(), w_box, pooler[0], 1.0 / C.STRIDE, pooler[1], pooler[2])
        bf = torch.zeros(C.N_ROWS, bf_live.shape[1], dtype=torch.float64).index_copy(0, live, bf_live)
        record_losses(out, "model/" + C.run_name(k, label, ent, mode), ref, dann, queue, feat, bf, mc["scores"], rois, mc["w_img"],
                      mc["w_ins"], C.WEIGHT_SETS[k], label, pooler, ent, mc["masks"] if mode == "train" else None,
                      extra_leaves={"w_box/" + n: v for n, v in w_box.items()})
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "entries")
    for k in sorted(out):
        if k.endswith("/value"):
            print(" ", k, out[k])


if __name__ == "__main__":
    main()
