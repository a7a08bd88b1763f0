"""Two gloo ranks on the CPU (the spawning pattern of tests/test_dist_gloo.py): step_amd.dist.BucketedReducer over a FlatSGD arena --
buckets all-reduced from autograd's hooks during backward, the averaging factor folded into FlatSGD.step(grad_scale=) -- leaves BOTH
ranks with the parameters of a single-process torch.optim.SGD on the whole batch, over two steps (the second runs the momentum
recurrence).  The optimizer's arenas live on the CPU through the test-only interpreter patch."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

KW = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv3d(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(4 * 2 * 4 * 4, 5))


def _data():
    torch.manual_seed(1)
    return torch.randn(6, 3, 2, 4, 4), torch.randn(6, 5)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from step_amd import dist as D
    from step_amd.optim import FlatSGD
    from tests.emul.patch import emulated_kernels
    D.init("gloo")
    clips, target = _data()
    model = _model()
    if rank == 1:                                  # replicas are made identical by the broadcast
        for p in model.parameters():
            p.data.add_(1.0)
    D.broadcast_parameters([model])
    idx = D.shard_clips(6, rank, world)
    with emulated_kernels():
        opt = FlatSGD(model.parameters(), **KW)
        red = D.BucketedReducer(opt, bucket_bytes=256)           # tiny buckets: several all-reduces
        nbuckets = len(red.buckets)
        scales = []
        for _ in range(2):
            red.begin()
            ((model(clips[idx]) - target[idx]) ** 2).mean().backward()
            f = red.finish()
            scales.append(f)
            opt.step(grad_scale=f, zero_grad=True)
        red.close()
        out = (opt.flat_param.numpy().copy(), opt.momentum_buffer.numpy().copy(), [(o, n) for _, _, o, n in opt._entries], nbuckets, scales,
               opt.step_count)
    q.put((rank, out))                             # numpy arrays travel by value
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_bucketed_exchange_over_flat_sgd_matches_single_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q), daemon=True) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=120) for _ in range(2))     # (a worker that died never answers: fail, do not wait for ever)
    except Exception:
        for p in procs:
            p.kill()
        raise AssertionError("a rank did not deliver its result (exit codes %s)" % [p.exitcode for p in procs])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    clips, target = _data()
    model = _model()
    ref = torch.optim.SGD(model.parameters(), **KW)
    for _ in range(2):
        ref.zero_grad()
        ((model(clips) - target) ** 2).mean().backward()     # equal shards: the mean of the rank means is the global mean
        ref.step()
    for rank in (0, 1):
        arena, buf, offs, nbuckets, scales, count = got[rank]
        assert nbuckets >= 3 and scales == [0.5, 0.5] and count == 2
        for (o, n), p in zip(offs, model.parameters()):
            assert np.allclose(arena[o:o + n], p.detach().reshape(-1).numpy(), rtol=1e-5, atol=1e-6), rank
            assert np.allclose(buf[o:o + n], ref.state[p]["momentum_buffer"].reshape(-1).numpy(), rtol=1e-5, atol=1e-6), rank
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])      # the replicas stay identical
