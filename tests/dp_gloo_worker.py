"""One rank of the two-process gloo test of tests/test_parallel_cpu.py (RANK, WORLD_SIZE, MASTER_ADDR and MASTER_PORT in the environment):
parallel.exchange over a CPU arena with seeded, rank-specific contents, then once more with a NaN in rank 1's tail slot 0; what each rank
holds afterwards goes to OUT/rank{r}.pt.  Not a test module."""
import datetime
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stmask_amd import parallel  # noqa: E402

SHAPES = [(3, 5), (0,), (7,), (2, 1, 3), (4099,)]


def fill(arena, rank, round_):
    g = torch.Generator().manual_seed(100 * round_ + rank)
    for v in arena.views:
        v.copy_(torch.randn(v.shape, generator=g) * 10.0 ** (rank - 1))
    arena.write_tail([torch.randn((), generator=g) for _ in range(arena.n_tail)])


def main(out):
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
    params = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    arena = parallel.GradArena(params, n_tail=8)
    got = {}
    fill(arena, rank, 0)
    got["local"] = arena.flat.clone()
    parallel.exchange(arena)
    got["summed"] = arena.flat.clone()
    fill(arena, rank, 1)
    if rank == 1:
        arena.tail[0] = float("nan")
    parallel.exchange(arena)
    got["poisoned"] = arena.flat.clone()
    got["first_difference_same"] = parallel.first_difference([torch.arange(5.0), torch.ones(3)])
    got["first_difference_rank"] = parallel.first_difference([torch.arange(5.0), torch.full((3,), float(rank)), torch.ones(2) * rank])
    t = [torch.full((4,), float(rank + 1)), torch.tensor([rank + 7])]
    parallel.broadcast_from_rank0(t)
    got["broadcast"] = t
    torch.save(got, os.path.join(out, f"rank{rank}.pt"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
