"""What the tests of handles bound with set_shard share: the host hook that carries their exchange steps, and one thread per rank."""
import threading


class Ring:
    """The host hook of `world` ranks: every rank brings its device buffer, the buffers are summed on the host (u64 wraps, as the
    device sum does) and every rank takes the sum back. A rank that waits in vain fails its call instead of hanging."""

    def __init__(self, world):
        import torch

        self.torch, self.world = torch, world
        self.barrier = threading.Barrier(world, timeout=60)
        self.bufs = [None] * world
        self.dtypes, self.calls = set(), 0

    def hook(self, rank):
        def allreduce(ptr, count, dtype):
            import scanrs_amd

            torch = self.torch
            self.dtypes.add(dtype)
            if rank == 0:
                self.calls += 1
            t = torch.as_tensor(scanrs_amd.DevArray(ptr, count, "<i8" if dtype == 1 else "<f8"), device="cuda:0")
            self.bufs[rank] = t.cpu().numpy()
            self.barrier.wait()
            total = self.bufs[0].copy()
            for b in self.bufs[1:]:
                total += b  # (int64 wraps like uint64)
            self.barrier.wait()
            t.copy_(torch.from_numpy(total))
            torch.cuda.synchronize()
            return 0

        return allreduce


def run_ranks(world, fn):
    """fn(rank) on one thread per rank, all joined: (results, exceptions), each with one entry per rank and None where the other holds."""
    out, err = [None] * world, [None] * world

    def work(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # noqa: BLE001
            err[r] = e

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return out, err
