"""worker of tests/test_gpu_image_cache.py::test_two_ranks_on_one_card: one data-parallel rank (both share cuda:0, gloo)
iterating its train and val loaders with and without the device image cache for 2 epochs; every batch must be equal.
usage: image_cache_dp_worker.py RANK WORLD PORT OUTDIR DEFN"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    rank, world, port, outdir, defn_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.yogo_dataloader import get_dataloader

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    defn = DatasetDefinition.from_yaml(defn_path)
    kw = dict(Sx=12, Sy=8, training=True, image_hw=(64, 96), device=dev)
    cached = get_dataloader(defn, 4, device_image_cache_gib=1.0, **kw)
    plain = get_dataloader(defn, 4, **kw)
    batches, order = 0, []
    for name in ("train", "val"):
        for e in range(2):
            got = []
            for dls in (cached, plain):
                dls[name].sampler.set_epoch(e)
                torch.manual_seed(100 * rank + e)
                got.append([(i.cpu(), l.cpu()) for i, l in dls[name]])
            assert len(got[0]) == len(got[1]) > 0, (name, e)
            for k, ((ci, cl), (pi, pl)) in enumerate(zip(*got)):
                assert torch.equal(ci, pi) and torch.equal(cl, pl), (rank, name, e, k)
            batches += len(got[0])
            if name == "train":
                order.append(list(iter(cached[name].sampler)))
    caches = [cached[name].cache for name in ("train", "val")]
    torch.save({"batches": batches, "order": order, "S": sum(c.S for c in caches), "resident": sum(int(c.resident.sum()) for c in caches)},
               os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
