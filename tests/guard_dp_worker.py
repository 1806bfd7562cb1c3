"""Worker of tests/test_gpu_grad_guard.py: one of two data-parallel ranks of a Trainer with ``grad_guard = "skip"``, launched by
torch.distributed.run over gloo so that both ranks can share the single GPU of the test box (as tests/dp_gpu_worker.py).  Rank 1
alone writes an inf into its gradient before the exchange; the summed buffer is the same on both ranks, so both must skip - with no
collective beyond the gradient's own."""
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from fusiondepth_amd import dp, synthetic
    from fusiondepth_amd.options import MonodepthOptions
    from fusiondepth_amd.trainer import Trainer
    out_path = sys.argv[1]
    rank, world, local_rank = dp.init_from_env()
    torch.cuda.set_device(0)
    H, W, B = 64, 96, 2
    opt = MonodepthOptions().parse(["--num_layers", "18", "--weights_init", "scratch", "--batch_size", str(B), "--height", str(H),
                                    "--width", str(W)])
    torch.manual_seed(100 + rank)                        # the broadcast of rank 0's state makes the replicas equal
    tr = Trainer(opt, rank=rank, world_size=world, verbose=False)
    tr.grad_guard = "skip"
    tr.grad_sync.overlap = False                         # one exchange of the whole buffer in finish(): "before the exchange" is a place

    def batch(step):
        b = synthetic.make_batch(B, H, W, seed=900 + step + 31 * rank)
        g = torch.Generator(device="cuda"); g.manual_seed(77 + step + 13 * rank)
        b["_noise"] = [torch.randn(B, 2, H, W, device="cuda", generator=g) for _ in range(4)]
        return b

    def checksum(p):
        p = p.double()
        return [float(p.sum()), float(p.abs().sum())]

    def step(k, inject):
        tr._forward_backward(batch(k), eager=True)       # Trainer.train_step, written out
        if inject:
            tr.flat.flat_grad[tr.flat.numel() // 2] = float("inf")
        scale = tr.grad_sync.finish()
        tr.optimizer_step(scale)
        tr._ensure_weight_plan()
        tr.step += tr.accumulate_step
        torch.cuda.synchronize()

    init = tr.flat.flat_param.clone()
    res = {"rank": rank, "injected": rank == 1, "before": checksum(init)}
    step(0, inject=rank == 1)
    res["report"] = tr.guard_report()
    res["stats_bits"] = tr.optim.guard_stats.view(torch.int64).tolist()
    res["unchanged"] = bool(torch.equal(tr.flat.flat_param.view(torch.int32), init.view(torch.int32)))
    res["grad_zero"] = float(tr.flat.flat_grad.abs().max()) == 0.0
    res["device_step"] = float(tr.optim.state[0])
    res["after"] = checksum(tr.flat.flat_param)
    res["finite"] = bool(torch.isfinite(tr.flat.flat_param).all())
    step(1, inject=False)                                # the next, finite step is taken by both
    res["device_step_next"] = float(tr.optim.state[0])
    res["moved_next"] = not torch.equal(tr.flat.flat_param, init)
    res["finite_next"] = bool(torch.isfinite(tr.flat.flat_param).all())
    res["after_next"] = checksum(tr.flat.flat_param)
    with open(out_path + ".%d" % rank, "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
