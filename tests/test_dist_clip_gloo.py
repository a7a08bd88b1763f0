"""Two gloo ranks on the CPU (the spawning pattern of tests/test_dist_gloo_sgd.py): the bucketed exchange over a FlatSGD arena followed by
step(grad_scale=1/world, max_grad_norm=m) -- the clip acts on the EXCHANGED gradient, so both ranks report the same total_norm bits, clip
by the same coefficient and hold the same parameters, those of a single-process torch.optim.SGD on the whole batch preceded by
torch.nn.utils.clip_grad_norm_, over two steps.  The optimizer's arenas live on the CPU through the test-only interpreter patch."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dist_gloo_sgd import KW, _data, _free_port, _model

MAX_NORM = 0.5                                     # below the norm of this problem's first gradients (asserted): both steps clip


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
        red = D.BucketedReducer(opt, bucket_bytes=256)
        stats = []
        for _ in range(2):
            red.begin()
            ((model(clips[idx]) - target[idx]) ** 2).mean().backward()
            f = red.finish()
            opt.step(grad_scale=f, zero_grad=True, max_grad_norm=MAX_NORM)
            stats.append(opt.grad_norm.numpy().copy())
        red.close()
        out = (opt.flat_param.numpy().copy(), opt.momentum_buffer.numpy().copy(), [(o, n) for _, _, o, n in opt._entries], stats, opt.step_count)
    q.put((rank, out))                             # numpy arrays travel by value
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_exchange_then_clip_matches_single_process():
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
    norms = []
    for _ in range(2):
        ref.zero_grad()
        ((model(clips) - target) ** 2).mean().backward()     # equal shards: the mean of the rank means is the global mean
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)))
        ref.step()
    assert min(norms) > MAX_NORM
    for rank in (0, 1):
        arena, buf, offs, stats, count = got[rank]
        assert count == 2
        for k in range(2):
            assert abs(float(stats[k][0]) - norms[k]) <= 1e-5 * norms[k] and stats[k][1] < 1.0 and stats[k][2] == 0.0, (rank, k, stats[k], norms[k])
        for (o, n), p in zip(offs, model.parameters()):
            assert np.allclose(arena[o:o + n], p.detach().reshape(-1).numpy(), rtol=1e-5, atol=1e-6), rank
            assert np.allclose(buf[o:o + n], ref.state[p]["momentum_buffer"].reshape(-1).numpy(), rtol=1e-5, atol=1e-6), rank
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0][3], got[1][3]))               # the same total_norm / coefficient bits
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])      # the replicas stay identical
