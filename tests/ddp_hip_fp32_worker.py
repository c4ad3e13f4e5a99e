"""Worker process of tests/test_hip_fp32_accum.py (not collected by pytest): the train step with grad_accum="fp32" under
DistributedDataParallel against the same step on the unwrapped model, in one process per rank.  Every rank runs the SAME
batch, so the average over ranks is each rank's own gradient exactly and the wrapped step must give the unwrapped step's bits:
gradients, updated weights, losses.  A communication hook counts the bucket all-reduces of every step (param.grad is None until
the last pass, so the reducer must see each bucket exactly once).  ``gloo`` with one rank runs on any GPU box; ``nccl`` (RCCL)
with one GPU per rank where there are two.  Rank 0 saves the results.

    RANK/WORLD_SIZE/MASTER_ADDR/MASTER_PORT from the environment;  argv: backend out_path gpus_available
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ddp_hip_worker import H, MINI, T, V, build_model   # noqa: E402  (also puts the repository and the oracle on sys.path)

ROWS, STEPS = 8, 2     # 4 micro-batches per step (> 2: the two-stream pipeline engages, the last pass runs isolated)


def run(backend, out_path, gpus):
    from omnibiote_amd import train_encoder as TE
    from omnibiote_amd.mup_compat import mu_param_groups
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = rank % max(gpus, 1) if backend == "nccl" else 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
    rng = np.random.default_rng(5)
    ids = torch.from_numpy(TE.synthetic_rows(ROWS, T, V, rng, single_document=False)).to(dev)
    mlm = torch.from_numpy(rng.random((ROWS, T)) < 0.15)
    mlm[MINI:2 * MINI] = False            # the second micro-batch has nothing masked: its readout node does not run
    mlm = mlm.to(dev)
    lr, wd = 1e-2, 1e-2
    results, bucket_calls, n_buckets = {}, [], 0
    for tag in ("plain", "ddp"):
        m = build_model(dev)
        model = m
        calls = []
        if tag == "ddp":
            model = TE.wrap_ddp(m, local, bucket_cap_mb=1)     # 1 MB buckets: several buckets even at this size

            def hook(state, bucket, calls=calls):
                calls.append(bucket.index())
                fut = dist.all_reduce(bucket.buffer().div_(world), async_op=True).get_future()
                return fut.then(lambda f: f.value()[0])

            model.register_comm_hook(None, hook)
        opt = TE.FusedAdamW(mu_param_groups(list(m.parameters()), lr, wd), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        step = TE.TrainStep(model, opt, None, mini_batch_size=MINI, n_head=H, pipeline_streams=2, grad_accum="fp32")
        losses = []
        for s in range(STEPS):
            before = len(calls)
            losses.append(step(ids, mlm_mask=mlm)["loss"].item())
            torch.cuda.synchronize()
            if tag == "ddp":
                bucket_calls.append(sorted(calls[before:]))
                n_buckets = max(n_buckets, max(calls) + 1)
        results[tag] = {"losses": losses, "g": {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()},
                        "w": {k: p.detach().cpu().clone() for k, p in m.named_parameters()}}
    if rank == 0:
        torch.save(dict(results, bucket_calls=bucket_calls, n_buckets=n_buckets, steps=STEPS), out_path)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2], int(sys.argv[3]))
