"""Worker of test_gpu_trainer.py::test_two_ranks_share_gpu_identical_tokens_and_a_shared_skip: run under torch.distributed.run with two
ranks on cuda:0 over gloo.  Every rank trains the same initial model on its own batches (rank 1's second batch is non-finite) and rank 0
writes what the test asserts to $LR_TRAINER_RANKS_OUT."""
import json
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    from test_gpu_trainer import _batches, _model, _tokens
    from leftrefill_amd.trainer import Trainer
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    m, cfg = _model()                                                   # same seed: the same initial tokens on every rank
    t0 = _tokens(m)
    batches = _batches(cfg, 4, bad_at=1 if rank == 1 else None, seed=5 + rank)
    root = os.path.join(os.getcwd(), f"run_rank{rank}")             # only rank 0 may write its checkpoint
    tr = Trainer(max_steps=4, precision=16, growth_interval=3, default_root_dir=root, local_rank=rank, verbose=False)
    torch.manual_seed(123 + rank)
    tr.fit(m, batches)
    dist.barrier()
    tok = _tokens(m).cpu()
    toks = [torch.empty_like(tok) for _ in range(2)]
    dist.all_gather(toks, tok)
    mine = [[int(f) for f in tr.found_inf_history], tr.optimizer.amp_state()["scale"], os.path.exists(os.path.join(root, "ckpts", "last.ckpt"))]
    every = [None, None]
    dist.all_gather_object(every, mine)
    if rank == 0:
        with open(os.environ["LR_TRAINER_RANKS_OUT"], "w") as f:
            json.dump({"world": dist.get_world_size(), "tokens_bit_identical": bool(torch.equal(toks[0], toks[1])),
                       "moved": float((toks[0] - t0.cpu()).abs().max()), "found_inf": [e[0] for e in every], "scale": [e[1] for e in every],
                       "ckpt_written_by": [e[2] for e in every]}, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
