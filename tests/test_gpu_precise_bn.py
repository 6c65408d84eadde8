"""TEST.PRECISE_BN on the device: sfod_bn_finalize_pop / sfod_bn_pop_commit / sfod_bn_pop_merge against the float64 definition
(tests/helpers/precise_bn_definitions.py), ``update_bn_stats`` against fvcore's literal procedure replayed on the momentum
path, the trainers' hook, and two ranks on one GPU.

Gates (derived, not measured).  Kernel level: everything is fp64 with one rounding to fp32, so running_mean is within
2^-23 (|mu| + sigma) and running_var within 2^-22 var of the definition evaluated on the SAME fp32 block statistics.  Module
level: fvcore's route passes the per-batch mean and unbiased variance through fp32 buffers (2^-24 relative each) before it
forms E[x^2] - E[x]^2, hence 2^-22 (|mu| + sigma) and 2^-21 (var + mu^2)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import precise_bn_definitions as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
HOT_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
SRC_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_source_new.yaml")
DA_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_da.yaml")
R101_YAML = os.path.join(CONFIGS, "r101_c4_cs_foggy_adaptive_teacher_source_free.yaml")
BAND, SENT = 8, -7.25


# ---- kernel level ------------------------------------------------------------------------------------------------------------
def stats_tensor(counts, sums, m2):
    """fp32 block statistics in the layout of a convolution epilogue: [blk][sum | centred square sum][c], then the counts"""
    flat = np.concatenate([np.stack([sums, m2], 1).reshape(-1), counts]).astype(np.float32)
    t = torch.from_numpy(flat).to(DEV)
    t.nblk = len(counts)
    return t


def make_passes(C, nblocks, seed, offset=0.0):
    """three passes with different row counts; some blocks are empty -> [(stats tensor, M, (M, mu_b, tot) definition)]"""
    rng = np.random.default_rng(seed)
    mu, sd = offset + rng.normal(size=C), 0.5 + rng.random(C)
    out = []
    for rows in (3, 1, 7):
        counts = rng.integers(0, 2 * rows + 1, size=nblocks)
        counts[0] = rows
        if nblocks > 1:
            counts[-1] = 0                                   # a block with count 0 in every pass
        bounds = np.concatenate([[0], np.cumsum(counts)])
        x = rng.normal(mu + 0.3 * rng.normal(size=C), sd, size=(int(bounds[-1]), C))
        bs = D.block_stats(x, bounds)
        out.append((stats_tensor(*bs), int(bounds[-1]), D.merge_blocks(*bs)))
    assert len({m for _, m, _ in out}) == 3                  # three different M: an unweighted rule cannot pass
    return out


def banded(n, dtype):
    """[BAND sentinel | n | BAND sentinel] -> (whole, the middle view)"""
    whole = torch.full((n + 2 * BAND,), SENT, dtype=dtype, device=DEV)
    return whole, whole[BAND:BAND + n]


def check_gates(label, rm, rv, acc):
    n, mean, m2 = acc
    var = m2 / n
    em = (np.abs(rm.double().cpu().numpy() - mean) / D.mean_gate(mean, var, 23)).max()
    ev = (np.abs(rv.double().cpu().numpy() - var) / (2.0 ** -22 * var)).max()
    print(f"[precise_bn {label}] worst error / gate: running_mean {em:.3g}, running_var {ev:.3g}")
    assert em <= 1.0 and ev <= 1.0, (label, em, ev)


KERNEL_CASES = [(64, 1, 1, 0.0), (72, 16, 1, 0.0), (64, 17, 1, 0.0), (72, 64, 1, 0.0), (72, 64, 0, 0.0), (64, 65, 1, 0.0),
                (64, 65, 0, 0.0), (72, 64 * 64 + 5, 1, 0.0), (72, 17, 1, 1000.0)]


@pytest.mark.parametrize("C,nblocks,fused,offset", KERNEL_CASES)
def test_finalize_pop_accumulates_and_commit_writes_the_population_statistics(native, C, nblocks, fused, offset):
    passes = make_passes(C, nblocks, seed=C + nblocks, offset=offset)
    C2 = 24                                                  # a second layer that never runs
    cols = BAND + C + C2 + BAND
    acc = torch.full((3, cols), SENT, dtype=torch.float64, device=DEV)
    acc[:, BAND:BAND + C + C2] = 0.0
    view = acc[:, BAND:BAND + C]
    rm_all, rm = banded(C, torch.float32)
    rv_all, rv = banded(C, torch.float32)
    rm2_all, rm2 = banded(C2, torch.float32)
    rv2_all, rv2 = banded(C2, torch.float32)
    nbt = torch.tensor(11, dtype=torch.int64, device=DEV)
    try:
        native.set_bn_finalize_fused(bool(fused))
        for stats, M, _ in passes:
            m0, i0 = native.bn_finalize(stats, M, C, rm, rv, 0.1, 1e-5, 0)
            m1, i1 = native.bn_finalize(stats, M, C, rm, rv, 0.1, 1e-5, 1, num_batches_tracked=nbt, pop=view)
            assert torch.equal(m0, m1) and torch.equal(i0, i1)           # bit-identical to sfod_bn_finalize
    finally:
        native.set_bn_finalize_fused(True)
    # nothing but the accumulator's own columns and the counter moved
    assert int(nbt) == 11 + 3
    assert (rm_all == SENT).all() and (rv_all == SENT).all()
    a = acc.cpu().numpy()
    assert (a[:, :BAND] == SENT).all() and (a[:, BAND + C + C2:] == SENT).all() and (a[:, BAND + C:BAND + C + C2] == 0).all()
    want = D.accumulate([p[2] for p in passes])
    assert (a[0, BAND:BAND + C] == want[0]).all()
    native.bn_pop_commit(acc, [(BAND, rm, rv), (BAND + C, rm2, rv2)])
    torch.cuda.synchronize()
    check_gates(f"C={C} nblocks={nblocks} fused={fused} offset={offset}", rm, rv, want)
    for whole in (rm_all, rv_all):
        assert (whole[:BAND] == SENT).all() and (whole[BAND + C:] == SENT).all()
    assert (rm2_all == SENT).all() and (rv2_all == SENT).all()         # n = 0: skipped
    assert torch.equal(acc.cpu(), torch.from_numpy(a))                  # the commit only reads the accumulator
    # an unweighted rule (the older fvcore one) does not pass these gates on these passes
    bad_m, bad_v = D.commit(D.accumulate([p[2] for p in passes], fault="unweighted"))
    var = want[2] / want[0]
    assert (np.abs(bad_m - want[1]) / D.mean_gate(want[1], var, 23)).max() > 1.0 or \
        (np.abs(bad_v - var) / (2.0 ** -22 * var)).max() > 1.0


def test_fp32_second_moment_would_fail_the_offset_case():
    """what the |mean| = 1000 sigma case is there for: E[x^2] - E[x]^2 formed in fp32 misses the variance gate by orders"""
    rng = np.random.default_rng(3)
    x = rng.normal(1000.0, 1.0, size=(4000, 4))
    e2 = np.float32((x.astype(np.float32) ** 2).mean(0, dtype=np.float32))
    e1 = np.float32(x.astype(np.float32).mean(0, dtype=np.float32))
    assert (np.abs((e2 - e1 * e1).astype(np.float64) - x.var(0)) / (2.0 ** -22 * x.var(0))).max() > 100.0


@pytest.mark.parametrize("C", [64, 72])
def test_pop_merge_of_two_halves_is_the_accumulator_of_the_whole(native, C):
    passes = make_passes(C, 17, seed=100 + C)

    def accumulate(subset):
        acc, (view,) = native.bn_pop_accumulator([C], DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        for stats, M, _ in subset:
            native.bn_finalize(stats, M, C, rm, rv, 0.1, 1e-5, 1, pop=view)
        return acc
    whole, a, b = accumulate(passes), accumulate(passes[:1]), accumulate(passes[1:])
    band = torch.full((3 * C + 2 * BAND,), SENT, dtype=torch.float64, device=DEV)
    dst = band[BAND:BAND + 3 * C].view(3, C)
    dst.copy_(a)
    b0 = b.clone()
    native.bn_pop_merge(dst, b)
    torch.cuda.synchronize()
    assert (band[:BAND] == SENT).all() and (band[BAND + 3 * C:] == SENT).all() and torch.equal(b, b0)
    assert torch.equal(dst[0], whole[0])
    want = D.accumulate([p[2] for p in passes])
    rm, rv = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    native.bn_pop_commit(dst.contiguous(), [(0, rm, rv)])
    check_gates(f"merge C={C}", rm, rv, want)
    rm_w, rv_w = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    native.bn_pop_commit(whole, [(0, rm_w, rv_w)])
    check_gates(f"whole C={C}", rm_w, rv_w, want)
    # an empty side changes nothing, in either position
    zero, _ = native.bn_pop_accumulator([C], DEV)
    keep = whole.clone()
    native.bn_pop_merge(keep, zero)
    native.bn_pop_merge(zero, whole)
    assert torch.equal(keep, whole) and torch.equal(zero, whole)


def test_bad_arguments_are_refused_before_any_launch(native):
    C = 64
    (stats, M, _), = make_passes(C, 4, seed=1)[:1]
    mean, invstd = torch.full((C,), SENT, device=DEV), torch.full((C,), SENT, device=DEV)
    rm, rv = torch.full((C,), SENT, device=DEV), torch.full((C,), SENT, device=DEV)
    ws = torch.empty(native.query("sfod_bn_finalize_ws_floats", C), dtype=torch.float32, device=DEV)
    acc = torch.full((3, 2 * C), SENT, dtype=torch.float64, device=DEV)

    def finalize(pop_ptr, stride):
        native.call("sfod_bn_finalize_pop", stats, stats.nblk, M, C, mean, invstd, rm, rv, 0.1, 1e-5, 1, None, ws, pop_ptr, stride)

    def commit(rows, stride=2 * C, pop=None):
        host = torch.tensor(rows, dtype=torch.int64)
        native.call("sfod_bn_pop_commit", acc.data_ptr() if pop is None else pop, stride, host.to(DEV), host.data_ptr(), len(rows))
    bad = [lambda: finalize(acc.data_ptr() + 4, 2 * C), lambda: finalize(acc.data_ptr(), 0), lambda: finalize(acc.data_ptr(), -2 * C),
           lambda: finalize(acc.data_ptr(), C - 1),
           lambda: commit([[C + 1, C, rm.data_ptr(), rv.data_ptr()]]), lambda: commit([[0, C, rm.data_ptr(), rv.data_ptr()],
                                                                                        [2 * C, 1, rm.data_ptr(), rv.data_ptr()]]),
           lambda: commit([[-1, C, rm.data_ptr(), rv.data_ptr()]]), lambda: commit([[0, C, 0, rv.data_ptr()]]),
           lambda: commit([[0, C, rm.data_ptr(), rv.data_ptr()]], stride=0),
           lambda: commit([[0, C, rm.data_ptr(), rv.data_ptr()]], pop=acc.data_ptr() + 4),
           lambda: native.call("sfod_bn_pop_merge", acc.data_ptr() + 4, acc, C),
           lambda: native.call("sfod_bn_pop_merge", acc, acc, C), lambda: native.call("sfod_bn_pop_merge", acc, acc[:, C:].contiguous(), -1)]
    for i, f in enumerate(bad):
        with pytest.raises(native.NativeLibraryError, match="code -1000"):
            f()
    torch.cuda.synchronize()
    for t in (mean, invstd, rm, rv, acc):
        assert (t == SENT).all()


# ---- module level ----------------------------------------------------------------------------------------------------------
def frames(n, seed, H=64, W=96):
    g = torch.Generator().manual_seed(seed)
    return [{"image": torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(DEV), "height": H, "width": W}
            for _ in range(n)]


def bn_buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def build(sfod, yaml, dtype, *opts):
    cfg = sfod.config.setup_cfg(yaml, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", dtype] + list(opts))
    torch.manual_seed(7)
    return cfg, sfod.modeling.build_model(cfg).train()


@pytest.mark.parametrize("arch,dtype", [("vgg", "fp32"), ("vgg", "bf16x3"), ("vgg", "f16x3"), ("r50", "fp32"), ("r50", "bf16x3"),
                                        ("r50", "f16x3")])
def test_update_bn_stats_agrees_with_fvcores_procedure_on_the_momentum_path(sfod, native, arch, dtype, monkeypatch):
    pb = sfod.engine.precise_bn
    if arch == "vgg":
        cfg, model = build(sfod, HOT_YAML, dtype)
    else:
        cfg, model = build(sfod, R101_YAML, dtype, "MODEL.RESNETS.DEPTH", "50")
    bb = model.backbone
    batches = [frames(2, 1), frames(1, 2), frames(3, 3)]
    live = {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert [m for m in live.values()] == pb.get_bn_modules(model) and len(live) >= 13
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    # fvcore: momentum 1.0, so that the running buffers hold the batch's own mean and unbiased variance after each pass
    rows = {}
    orig = native.bn_finalize

    def recording(stats, M, C, running_mean, *a, **k):
        rows[running_mean.data_ptr()] = M
        return orig(stats, M, C, running_mean, *a, **k)
    monkeypatch.setattr(native, "bn_finalize", recording)
    bb.bn_momentum = 1.0
    per_pass = []
    with torch.no_grad():
        for b in batches:
            model._features(model.preprocess_image(b))
            per_pass.append({n: (m.running_mean.double().cpu().numpy(), m.running_var.double().cpu().numpy(),
                                 float(rows[m.running_mean.data_ptr()])) for n, m in live.items()})
    bb.bn_momentum = 0.1
    monkeypatch.setattr(native, "bn_finalize", orig)
    model.load_state_dict(sd0)
    assert pb.update_bn_stats(model, batches, 3) == len(live)
    torch.cuda.synchronize()
    assert bb.bn_population is None and bb.bn_momentum == 0.1
    worst = (0.0, 0.0, "")
    for n, m in live.items():
        pm, pv = D.fvcore_population(*zip(*[per_pass[i][n] for i in range(3)]))
        em = (np.abs(m.running_mean.double().cpu().numpy() - pm) / D.mean_gate(pm, pv, 22)).max()
        ev = (np.abs(m.running_var.double().cpu().numpy() - pv) / (2.0 ** -21 * (pv + pm * pm))).max()
        worst = max(worst, (max(em, ev), min(em, ev), n))
        assert em <= 1.0 and ev <= 1.0, f"{arch} {dtype} layer {n}: mean error / gate {em:.3g}, variance error / gate {ev:.3g}"
        assert int(m.num_batches_tracked) == int(sd0[n + ".num_batches_tracked"]) + 3 and m.momentum == 0.1
    print(f"[precise_bn module {arch} {dtype}] {len(live)} layers, worst error / gate {worst[0]:.3g} ({worst[2]})")
    # parameters and everything frozen: untouched
    moved = {k for k, v in model.state_dict().items() if not torch.equal(v, sd0[k])}
    assert moved == {n + s for n in live for s in (".running_mean", ".running_var", ".num_batches_tracked")}
    precise = bn_buffers(model)
    # AdaBN with population statistics: the same passes, the same buffers; no reset needed
    model.load_state_dict(sd0)
    sfod.engine.adabn_refinement(cfg, model, batches, max_iters=2, precise=True)
    assert all(torch.equal(v, precise[k]) for k, v in bn_buffers(model).items())
    # ... and the default AdaBN path still is the momentum tail (reset, three updates)
    model.load_state_dict(sd0)
    sfod.engine.adabn_refinement(cfg, model, batches, max_iters=2)
    tail = bn_buffers(model)
    assert any(not torch.equal(tail[k], precise[k]) for k in tail if k.endswith("running_var"))
    assert all(int(v) == 3 + int(sd0[k]) for k, v in tail.items() if k.endswith("num_batches_tracked") and k[:-20] in live)


# ---- trainer level -----------------------------------------------------------------------------------------------------------
SMALL = ["SFOD.COMPUTE_DTYPE", "fp32", "SOLVER.IMS_PER_BATCH", "2", "SOLVER.IMS_PER_BATCH_TARGET", "2", "SFOD.SYNTHETIC.HEIGHT", "64",
         "SFOD.SYNTHETIC.WIDTH", "96", "SFOD.SYNTHETIC.NUM_IMAGES", "4", "INPUT.MIN_SIZE_TRAIN", "(64,)", "SFOD.DETERMINISTIC", "True",
         "SOLVER.MAX_ITER", "4", "TEST.EVAL_PERIOD", "2", "SOLVER.CHECKPOINT_PERIOD", "2", "TEST.PRECISE_BN.NUM_ITER", "3",
         "SFOD.EVAL_HOOK", "False", "TEST.VAL_LOSS", "False", "SEED", "5"]


def run_trainer(sfod, yaml, out_dir, enabled, *opts):
    """train() for MAX_ITER steps -> (trainer, image ids of the training batches, [(model state before, BN buffers after)] per
    update)"""
    cfg = sfod.config.setup_cfg(yaml, SMALL + ["OUTPUT_DIR", out_dir, "TEST.PRECISE_BN.ENABLED", str(enabled)] + list(opts))
    torch.manual_seed(5)
    tr = sfod.engine.get_trainer_class(cfg)(cfg)
    seen, updates = [], []
    inner = tr._data_loader_iter

    class Recording:
        def __next__(self):
            data = next(inner)
            lists = data if isinstance(data, tuple) else (data,)
            seen.append([[int(d["image_id"]) for d in lst] + [int(d["image"].sum()) for d in lst] for lst in lists])
            return data
    tr._data_loader_iter = Recording()
    orig = tr._do_precise_bn

    def recorded():
        before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
        orig()
        updates.append((tr.iter + 1, before, bn_buffers(tr.model)))
    tr._do_precise_bn = recorded
    tr.train()
    torch.cuda.synchronize()
    return cfg, tr, seen, updates


def replay(sfod, tr, before, batches, num_iters):
    tr.model.load_state_dict(before)
    sfod.engine.precise_bn.update_bn_stats(tr.model, batches, num_iters)
    return bn_buffers(tr.model)


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_base_trainer_runs_the_update_before_the_checkpointer_and_leaves_training_alone(sfod, native, tmp_path):
    out_off, out_on = str(tmp_path / "off"), str(tmp_path / "on")
    _, tr0, seen0, upd0 = run_trainer(sfod, SRC_YAML, out_off, False)
    cfg, tr, seen, upd = run_trainer(sfod, SRC_YAML, out_on, True)
    assert type(tr) is sfod.engine.BaseTrainer and upd0 == [] and tr0._precise_bn_loader is None
    assert [u[0] for u in upd] == [2, 4] and len(seen) == 4
    # training itself: the same batches, the same parameters and momentum buffers, bit for bit
    assert seen == seen0
    for (n, p), (n0, p0) in zip(tr.model.named_parameters(), tr0.model.named_parameters()):
        assert n == n0 and torch.equal(p.detach(), p0.detach()), n
    assert torch.equal(tr.optimizer.mom, tr0.optimizer.mom)
    assert not same(bn_buffers(tr.model), bn_buffers(tr0.model))
    # the statistics: a replay of update_bn_stats on a fresh second loader, which the second period CONTINUES
    final = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    second = iter(tr.build_train_loader(cfg))
    assert same(replay(sfod, tr, upd[0][1], second, 3), upd[0][2])
    assert same(replay(sfod, tr, upd[1][1], second, 3), upd[1][2])
    assert not same(replay(sfod, tr, upd[1][1], iter(tr.build_train_loader(cfg)), 3), upd[1][2])      # a restarted stream differs
    tr.model.load_state_dict(final)
    assert same(bn_buffers(tr.model), upd[1][2])
    # the checkpoint of iteration 2 (model_0000001) was written after the update
    ck = torch.load(os.path.join(out_on, "model_0000001.pth"), map_location=DEV, weights_only=False)["model"]
    assert all(torch.equal(torch.as_tensor(ck[k]).to(DEV), v) for k, v in upd[0][2].items())
    ck0 = torch.load(os.path.join(out_off, "model_0000001.pth"), map_location=DEV, weights_only=False)["model"]
    assert any(not torch.equal(torch.as_tensor(ck0[k]).to(DEV), v) for k, v in upd[0][2].items() if k.endswith("running_var"))


def test_source_free_trainer_updates_the_student_on_the_weak_half(sfod, native):
    cfg, tr, seen, upd = run_trainer(sfod, HOT_YAML, "", True, "WEAK_STRONG_AUGMENT", "True", "SFOD.SYNTHETIC.STRONG_AUGMENT", "True")
    assert type(tr) is sfod.engine.SourceFreeAdaptiveTeacherTrainer and [u[0] for u in upd] == [2, 4]
    second = iter(tr.build_train_loader(cfg))
    pairs = [next(second) for _ in range(6)]
    assert all(isinstance(p, tuple) and len(p) == 2 for p in pairs)
    assert any(not torch.equal(s["image"], w["image"]) for s, w in zip(pairs[0][0], pairs[0][1]))       # the halves do differ
    assert same(replay(sfod, tr, upd[0][1], [p[1] for p in pairs[:3]], 3), upd[0][2])
    assert same(replay(sfod, tr, upd[1][1], [p[1] for p in pairs[3:]], 3), upd[1][2])
    assert not same(replay(sfod, tr, upd[0][1], [p[0] for p in pairs[:3]], 3), upd[0][2])


def test_da_trainer_updates_on_both_domains_source_first(sfod, native):
    cfg, tr, seen, upd = run_trainer(sfod, DA_YAML, "", True)
    assert type(tr) is sfod.engine.DATrainer and [u[0] for u in upd] == [2, 4]
    second = iter(tr.build_train_loader(cfg))
    pairs = [next(second) for _ in range(6)]
    flat = lambda ps: [lst for p in ps for lst in p]              # source, target, source, target, ...: six passes of lists
    assert same(replay(sfod, tr, upd[0][1], flat(pairs[:3]), 6), upd[0][2])
    assert same(replay(sfod, tr, upd[1][1], flat(pairs[3:]), 6), upd[1][2])
    assert not same(replay(sfod, tr, upd[0][1], [p[0] for p in pairs[:3]], 3), upd[0][2])                # the source alone is not it
    nbt = [v for k, v in upd[0][2].items() if k.endswith("num_batches_tracked")]
    assert all(int(v) == 2 * 2 + 6 for v in nbt)          # two steps over both domains, then three batches of two passes


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------
WORKER = os.path.join(ROOT, "tests", "helpers", "two_rank_precise_bn_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_sync_gives_the_union_and_no_sync_each_ranks_share(tmp_path):
    port, procs = _free_port(), []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("MASTER_ADDR", None)
        log = open(os.path.join(tmp_path, f"rank{r}.log"), "w")
        procs.append((subprocess.Popen([sys.executable, WORKER, "--out", str(tmp_path), "--port", str(port)], env=env, stdout=log,
                                       stderr=subprocess.STDOUT), log))
    codes = []
    try:
        for p, log in procs:
            codes.append(p.wait(timeout=300))
    finally:
        for p, log in procs:
            if p.poll() is None:
                p.kill()          # exactly the children started above
            log.close()
    if any(codes):
        tails = "\n".join(open(os.path.join(tmp_path, f"rank{r}.log")).read()[-3000:] for r in range(2))
        pytest.fail(f"worker exit codes {codes}\n{tails}")
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False) for r in range(2))
    assert r0["columns"] == r1["columns"] and len(r0["layers"]) == 13
    # SYNC True: identical bits on both ranks, the definition over the union within the kernel-level gates
    assert all(torch.equal(r0["sync"][k], r1["sync"][k]) for k in r0["sync"])
    a0, a1 = r0["own_acc"].numpy(), r1["own_acc"].numpy()
    assert not np.array_equal(a0[1], a1[1]) and (a0[0] != a1[0]).all()          # different frames, different sizes
    union = D.chan_merge(tuple(a0), tuple(a1))
    off = 0
    for name, C in r0["layers"]:
        sl = slice(off, off + C)
        check_gates(f"two ranks union {name}", r0["sync"][name + ".running_mean"], r0["sync"][name + ".running_var"],
                    tuple(u[sl] for u in union))
        for r, a in ((r0, a0), (r1, a1)):       # SYNC False: each rank the statistics of its own share
            check_gates(f"two ranks own {name} rank {r['rank']}", r["own"][name + ".running_mean"], r["own"][name + ".running_var"],
                        tuple(u[sl] for u in a))
        off += C
    assert any(not torch.equal(r0["own"][k], r1["own"][k]) for k in r0["own"] if k.endswith("running_mean"))
    assert all(int(v) == int(r0["nbt0"]) + 2 for k, v in r0["sync"].items() if k.endswith("num_batches_tracked"))
