"""The bf16 gradient wire over TWO gloo ranks on the CPU: kernels on the host interpreter (tests/emul), tensors on the host.

The ranks hold different seeded gradients and the weights 2 and 3.  After the exchange both ranks must hold, bit for bit,
    widen(rne(widen(w0) + widen(w1)))
with w_r the numpy restatement's pack of rank r at its weight (tests/wire_cases.py; gloo sums two bfloat16 tensors as one float32 addition
and one round-to-nearest-even), and each rank's residual must be the restatement's.  A weight of 3 does not multiply exactly, so the
restatement forms 3 g + r in float64 -- where the sum is exact, which the test asserts with an error-free transformation -- and rounds
once, as the kernel's fused multiply-add does."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import wire_cases as WC

WEIGHTS = (2.0, 3.0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _grad(numel, rank, step):
    rs = np.random.RandomState(1000 + 10 * step + rank)
    return (rs.randn(numel) * np.exp(rs.randn(numel))).astype(np.float32)


def _worker(rank, world, port, q):
    try:
        _body(rank, world, port, q)
    except BaseException:                                        # the parent must hear about it
        import traceback
        q.put((rank, {"error": traceback.format_exc()[-3000:]}))
        raise


def _body(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from step_amd import dist as D
    from tests.emul.patch import emulated_kernels
    assert D.init("gloo") == (rank, world)
    out = {}
    with emulated_kernels():
        model, opt, wire, red, raw = WC._toy("cpu", bucket_bytes=256)
        assert red.active and len(red.buckets) >= 3
        out["numel"] = opt.numel
        # (a) two steps of allreduce_flat with hand-made gradients, the residual carried; tiny chunks in the second
        for step, chunk in ((0, 512 << 20), (1, 70)):
            opt.flat_grad.copy_(torch.from_numpy(_grad(opt.numel, rank, step)))
            f = D.allreduce_flat(opt.flat_grad, weight=WEIGHTS[rank], chunk_bytes=chunk, wire=wire)
            out["flat%d" % step] = (opt.flat_grad.numpy().copy(), wire.residual.numpy().copy(), f)
        # (b) the same through the bucketed reducer: the toy model's backward on this rank's clips, the residual of (a) carried on
        x, y = WC.toy_batch("cpu", seed=20 + rank)
        opt.zero_grad()
        red.begin(weight=WEIGHTS[rank])
        ((model(x) - y) ** 2).mean().backward()
        during = red.issued_during_backward
        f = red.finish()
        out["bucketed"] = (raw.numpy().copy(), opt.flat_grad.numpy().copy(), wire.residual.numpy().copy(), f, during, len(red.buckets))
        # (c) rank 1 has weight 0: it sends exact zeros and keeps its residual
        opt.flat_grad.copy_(torch.from_numpy(_grad(opt.numel, rank, 2)))
        before = wire.residual.numpy().copy()
        f = D.allreduce_flat(opt.flat_grad, weight=(2.0, 0.0)[rank], wire=wire)
        out["zero"] = (opt.flat_grad.numpy().copy(), wire.residual.numpy().copy(), before, f)
        red.close()
    q.put((rank, out))                                           # numpy arrays travel by value
    dist.barrier()
    dist.destroy_process_group()


def _fma32(g, s, r):
    """float32(g * s + r) with ONE rounding: the float64 sum is exact (checked), so the only rounding is the last one"""
    a, b = g.astype(np.float64) * s, r.astype(np.float64)
    t = a + b
    bb = t - a
    assert np.all((a - (t - bb)) + (b - bb) == 0), "the float64 sum is not exact: the restatement would double-round"
    return t.astype(np.float32)


def _pack(g, r, s):
    v = _fma32(g, s, r)
    w = WC.rne(v)
    return w, (v - WC.widen(w)).astype(np.float32)


def _summed(w0, w1):
    return WC.widen(WC.rne(WC.widen(w0) + WC.widen(w1)))


@pytest.mark.timeout(120)
def test_two_rank_bf16_wire_matches_the_restatement():
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get() for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in range(2):
        assert "error" not in got[r], got[r]["error"]
    numel = got[0]["numel"]
    res = [np.zeros(numel, np.float32), np.zeros(numel, np.float32)]
    # (a) two steps; the residuals differ per rank and are carried
    for step in range(2):
        ws = []
        for r in range(2):
            w, res[r] = _pack(_grad(numel, r, step), res[r], WEIGHTS[r])
            ws.append(w)
        want = _summed(*ws)
        for r in range(2):
            flat, residual, f = got[r]["flat%d" % step]
            assert f == 1.0 / 5.0
            assert np.array_equal(WC.bits(flat), WC.bits(want)), (step, r)
            assert np.array_equal(WC.bits(residual), WC.bits(res[r])), (step, r)
        assert np.any(res[0] != res[1]) and np.any(res[0] != 0)
    # (b) the bucketed reducer: same arithmetic on each rank's own backward gradient
    ws = []
    for r in range(2):
        raw = got[r]["bucketed"][0]
        assert np.abs(raw).max() > 0
        w, res[r] = _pack(raw, res[r], WEIGHTS[r])
        ws.append(w)
    want = _summed(*ws)
    for r in range(2):
        _, flat, residual, f, during, nb = got[r]["bucketed"]
        assert abs(f - 0.2) < 1e-7 and nb >= 3 and during >= 1
        assert np.array_equal(WC.bits(flat), WC.bits(want)), r
        assert np.array_equal(WC.bits(residual), WC.bits(res[r])), r
    # (c) weight 0 on rank 1: exact zeros on its wire, its residual as it was
    w0, res0 = _pack(_grad(numel, 0, 2), res[0], 2.0)
    want = _summed(w0, np.zeros(numel, np.uint16))
    for r in range(2):
        flat, residual, before, f = got[r]["zero"]
        assert f == 0.5
        assert np.array_equal(WC.bits(flat), WC.bits(want)), r
    assert np.array_equal(WC.bits(got[0]["zero"][1]), WC.bits(res0))
    assert np.array_equal(WC.bits(got[1]["zero"][1]), WC.bits(got[1]["zero"][2])) and np.array_equal(WC.bits(got[1]["zero"][1]), WC.bits(res[1]))
