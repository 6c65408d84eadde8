"""One rank of tests/test_gpu_precise_bn.py::test_two_ranks_sync_gives_the_union_and_no_sync_each_ranks_share: both ranks on
``cuda:0`` over gloo (RCCL refuses two ranks on one device), the hot yaml's model with the same weights on both ranks,
DIFFERENT frames per rank (three on rank 0, five on rank 1, two batches each).  ``update_bn_stats`` runs twice from the
same state: ``sync=False`` (the rank's own accumulator is recorded as it is committed) and ``sync=True``.  Started as a
fresh interpreter by the test; writes ``<out>/rank<r>.pt`` for the parent, which evaluates the definition."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--port", type=int, required=True)
    args = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{}".format(args.port), rank=rank, world_size=world)
    sfod = importlib.import_module("simple-sfod_amd")
    native = sfod.native
    native.load()
    yaml = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
    cfg = sfod.config.setup_cfg(yaml, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", "fp32"])
    torch.manual_seed(7)                                   # the same weights on both ranks
    model = sfod.modeling.build_model(cfg).train()

    def frames(n, seed, H=64, W=96):
        g = torch.Generator().manual_seed(seed)
        return [{"image": torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).cuda(), "height": H, "width": W}
                for _ in range(n)]
    batches = [frames(2, 10), frames(1, 11)] if rank == 0 else [frames(3, 20), frames(2, 21)]
    bns = [(n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def buffers():
        return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()
                if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    committed = []
    orig = native.bn_pop_commit

    def recording(acc, layers):
        committed.append(acc.detach().cpu().clone())
        return orig(acc, layers)
    native.bn_pop_commit = recording
    sfod.engine.update_bn_stats(model, batches, 2, sync=False)
    own = buffers()
    model.load_state_dict(sd0)
    sfod.engine.update_bn_stats(model, batches, 2, sync=True)
    synced = buffers()
    torch.cuda.synchronize()
    torch.save({"rank": rank, "layers": [(n, m.num_features) for n, m in bns], "columns": committed[0].shape[1],
                "own_acc": committed[0], "sync_acc": committed[1], "own": own, "sync": synced,
                "nbt0": int(sd0[bns[0][0] + ".num_batches_tracked"])}, os.path.join(args.out, "rank{}.pt".format(rank)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
