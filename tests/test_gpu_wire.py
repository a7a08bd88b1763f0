"""The bf16 gradient wire on the real gfx950 library: the cases of tests/wire_cases.py (shared with the interpreter run of
tests/test_emul_wire.py) plus what only exists on the device -- a size beyond one pass of the grid, pack + unpack replayed from a HIP
graph, two ranks training the toy model over the wire, and the launcher's --grad-wire switch."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import wire_cases as WC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", WC.KERNEL_CASES + WC.KERNEL_GPU_ONLY)
def test_gpu_wire_kernel(name, bk, golden):
    getattr(WC, name)(bk, golden)


@pytest.mark.parametrize("name", WC.MODULE_CASES)
def test_gpu_wire_module(name, golden):
    getattr(WC, name)("cuda", golden)


def test_pack_unpack_replayed_from_a_graph():
    """step_grad_pack16 + step_grad_unpack16 captured in a HIP graph on a plain stream (no process group takes part) and replayed three
    times with the gradient buffer rewritten between the replays: wire, gradient and residual match the restatement with the residual
    carried from replay to replay -- the calls take no host scalar that changes between steps."""
    import ctypes

    from step_amd import _capi, _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n = 65536 + 3
    grad = torch.zeros(n, device=dev)
    res = torch.zeros(n, device=dev)
    wire = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def both():
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(L.step_grad_pack16(_capi.BF16, ptr(grad), ptr(res), ptr(wire), n, 1.0, st), "step_grad_pack16")
        _capi.check(L.step_grad_unpack16(_capi.BF16, ptr(wire), ptr(grad), n, st), "step_grad_unpack16")

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        both()                                                   # recorded, not run
    torch.cuda.synchronize()
    assert not res.any() and not wire.view(torch.int16).any()
    r = np.zeros(n, np.float32)
    for k in range(3):
        gk = WC.gradients(n, 300 + k)
        grad.copy_(torch.from_numpy(gk))
        g.replay()
        torch.cuda.synchronize()
        v, want_w, r = WC.restate_pack(gk, r)
        got_w = wire.view(torch.int16).cpu().numpy().view(np.uint16)
        assert WC.same_wire(got_w, want_w, v), k
        assert np.array_equal(WC.bits(res.cpu().numpy()), WC.bits(r)), k
        assert np.array_equal(grad.cpu().numpy().view(np.uint32), got_w.astype(np.uint32) << np.uint32(16)), k
    assert np.any(r != 0)


LR, STEPS = 2.0 ** -7, 3


def _worker(rank, world, port, q):
    try:
        _body(rank, world, port, q)
    except BaseException:                                        # the parent must hear about it (a dead worker would leave it waiting)
        import traceback
        q.put((rank, {"error": traceback.format_exc()[-3000:]}))
        raise


def _body(rank, world, port, q):
    import torch.distributed as dist
    from step_amd import dist as D

    # >= 2 GPUs visible: one rank per GPU over RCCL; the 1-GPU box shares its GPU between the ranks over gloo (tests/test_gpu_ddp.py)
    if torch.cuda.device_count() >= world:
        dev = torch.device("cuda", rank)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world, device_id=dev)
    else:
        dev = torch.device("cuda:0")
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    out = {"backend": dist.get_backend(), "staged": False}
    orig = dist.all_reduce
    if dist.get_backend() == "gloo":
        # should this gloo build refuse bfloat16 DEVICE tensors (its host path takes them: tests/test_dist_wire_gloo.py), the wire is
        # staged through a host copy HERE, in the test's worker; the product is not touched
        try:
            orig(torch.zeros(8, dtype=torch.bfloat16, device=dev))
            torch.cuda.synchronize()
        except RuntimeError:
            dist.all_reduce = WC.host_staged(orig)
            out["staged"] = True
    model, opt, wire, red, raw = WC._toy(str(dev), bucket_bytes=256)
    assert red.active and len(red.buckets) >= 3
    out["p0"] = opt.flat_param.cpu().numpy()
    out["raw"], out["param"], out["residual"] = [], [], []
    for k in range(STEPS):
        x, y = WC.toy_batch(str(dev), seed=30 + 10 * k + rank)
        f = WC._backward(model, opt, x, y, red)
        assert f == 0.5
        out["raw"].append(raw.cpu().numpy())
        opt.step(grad_scale=f, zero_grad=True)
        torch.cuda.synchronize()
        out["param"].append(opt.flat_param.cpu().numpy())
        out["residual"].append(wire.residual.cpu().numpy())
    red.close()
    dist.all_reduce = orig
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_train_the_toy_model_over_the_bf16_wire():
    """Two ranks (RCCL with one rank per GPU where two are visible, else gloo on the shared cuda:0), the toy model under FlatSGD(lr = 2^-7,
    momentum 0) with a feedback wire and 256-byte buckets, three eager steps on different clips per rank.  After every step the ranks'
    flat_param are bit-identical to each other and to a single-process restatement of the same steps: each rank's recorded backward
    gradient packed by the numpy restatement with its own carried residual, the two wires summed as one float32 addition rounded to
    bfloat16, p -= 2^-7 * (0.5 * sum) -- both factors powers of two, so the update has one rounding however the compiler contracts it."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=240) for _ in range(2))
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    for r in range(2):
        assert "error" not in got[r], got[r]["error"]
    assert all(p.exitcode == 0 for p in procs)
    print("two-rank wire: backend %s, wire staged through the host in the worker: %s" % (got[0]["backend"], got[0]["staged"]))
    assert np.array_equal(got[0]["p0"], got[1]["p0"])
    p = got[0]["p0"].copy()
    res = [np.zeros_like(p), np.zeros_like(p)]
    for k in range(STEPS):
        ws = []
        for r in range(2):
            _, w, res[r] = WC.restate_pack(got[r]["raw"][k], res[r])
            ws.append(w)
        summed = WC.widen(WC.rne(WC.widen(ws[0]) + WC.widen(ws[1])))
        p = (p - np.float32(LR) * (summed * np.float32(0.5))).astype(np.float32)
        assert np.array_equal(WC.bits(got[0]["param"][k]), WC.bits(got[1]["param"][k])), k
        assert np.array_equal(WC.bits(got[0]["param"][k]), WC.bits(p)), k
        for r in range(2):
            assert np.array_equal(WC.bits(got[r]["residual"][k]), WC.bits(res[r])), (k, r)
    assert np.any(p != got[0]["p0"]) and np.any(res[0] != res[1])


def _launch(world, *args):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    two = torch.cuda.device_count() >= 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "train_step_amd.py"), "--iters", "3", "--warmup-iters", "2", "--log-every", "0"]
    cmd += list(args) + ([] if (two or world == 1) else ["--backend", "gloo"])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    summ = [ln for ln in lines if ln.get("summary")]
    assert len(summ) == 1, r.stdout[-2000:]
    return summ[0], [ln["param_checksum"] for ln in lines if "param_checksum" in ln]


@pytest.mark.timeout(900)
def test_train_step_amd_launcher_grad_wire_switch():
    """train_step_amd.py --grad-wire bf16 with two ranks, launched as tests/test_gpu_ddp.py launches its two-rank run, in the default capture
    form: the summary names the wire, exchange_bytes_per_step is half that of an --grad-wire fp32 run, the loss is finite and positive, and
    both ranks print the same param_checksum -- replicas that applied the same exchanged gradients."""
    s, sums = _launch(2, "--grad-wire", "bf16")
    assert s["grad_wire"] == "bf16" and s["world_size"] == 2 and s["adam_steps"] == 5
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0
    assert s["launch"].startswith("hipGraph replay") and "split" in s["launch"] and s["gradient_exchange"] is not None
    assert len(sums) == 2 and sums[0] == sums[1] and np.isfinite(sums[0]), sums
    s32, sums32 = _launch(1, "--grad-wire", "fp32")
    assert s32["grad_wire"] == "fp32" and len(sums32) == 1
    assert s["exchange_bytes_per_step"] * 2 == s32["exchange_bytes_per_step"] and s["exchange_bytes_per_step"] > 0
