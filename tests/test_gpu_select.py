"""The device-side proposal selection on the real gfx950 library: the cases of tests/select_cases.py (shared with the interpreter run of
tests/test_emul_select.py) plus what only exists on the device -- the training iteration with the selection inside ONE captured graph
and the launcher's --select-device switch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import select_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", SC.KERNEL_CASES)
def test_gpu_select_kernel(name, bk, golden):
    getattr(SC, name)(bk, golden)


@pytest.mark.parametrize("name", SC.MODULE_CASES)
def test_gpu_select_module(name, golden):
    getattr(SC, name)("cuda", golden)


def _run(mode, dropout, steps=4, warm=2):
    from step_amd import workloads

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    w = workloads.C4SelectTrainStep(dev, batch=1, seed=123, dtype=torch.bfloat16, capturable=(mode == "graph"), dropout=dropout, rng_seed=9,
                                    selection="device")
    assert w.rng.get_state() == (9, 0)
    p0 = w.opt.flat_param.clone()
    losses, picks = [], []

    def note(loss):
        losses.append(float(loss))
        picks.append((w.select_counts().copy(), [f.cpu().numpy().copy() for f in w.s_flat], list(w.selected)))
        assert w.selection_ran == "device"

    if mode == "graph":
        w.capture(warmup=warm)
        assert w.graph_mode == "select-one" and w.graph is not None and w._gB is None and w._g_update is None
        assert w.rng.offset() == warm * (3 + (9 if dropout else 0))              # the recording itself draws nothing
        for _ in range(steps - warm):
            note(w.step())
    else:
        for i in range(steps):
            loss = w.step_padded()
            if i >= warm:
                note(loss)
    torch.cuda.synchronize()
    out = ((w.opt.flat_param - p0).cpu().numpy(), np.array(losses), w.rng.offset(), w.opt.step_count, picks)
    del w
    torch.cuda.empty_cache()
    return out


def test_device_selection_step_is_one_graph_and_bit_identical():
    """C4SelectTrainStep(selection="device", bf16, batch 1, dropout 0.3, rng_seed 9), 4 iterations of which 2 warm up: step_padded() and
    capture() give the same losses and the same parameter delta bit for bit (same kernels on the same buffers, same draws: same seed,
    same offsets); the captured form is ONE graph ("select-one"); every iteration uses 9 dropout offsets + 3 selection offsets, so the
    generator ends at 4 x 12 (4 x 3 with dropout 0); two captured runs from one seed are identical; the selection changes from
    iteration to iteration (counts or selected rows); `selected` is the row total of `counts`; the losses are finite."""
    steps = 4
    padded, graph, again = _run("padded", 0.3), _run("graph", 0.3), _run("graph", 0.3)
    plain = _run("padded", 0.0)
    assert padded[2] == graph[2] == again[2] == steps * (9 + 3) and plain[2] == steps * 3
    assert padded[3] == graph[3] == steps
    assert np.isfinite(graph[1]).all() and np.isfinite(plain[1]).all() and np.abs(graph[0]).max() > 0
    print("device selection: losses padded %s graph %s, rows per step %s" % (padded[1].tolist(), graph[1].tolist(), [p[2] for p in graph[4]]))
    assert np.array_equal(padded[1], graph[1]), (padded[1], graph[1])
    assert np.array_equal(padded[0], graph[0])
    assert np.array_equal(graph[0], again[0]) and np.array_equal(graph[1], again[1])
    for (ca, ra, sa), (cb, rb, sb) in zip(padded[4], graph[4]):
        assert np.array_equal(ca, cb) and all(np.array_equal(x, y) for x, y in zip(ra, rb)) and sa == sb
        assert sa == [[int(v) for v in c.sum(axis=1)] for c in ca] and all(0 < n <= 15 for s_ in sa for n in s_)
    (c0, r0, _), (c1, r1, _) = graph[4]
    assert not (np.array_equal(c0, c1) and all(np.array_equal(x, y) for x, y in zip(r0, r1))), "two replays selected the same rows: the offset did not advance in the graph"


def test_host_selection_stays_the_default():
    """selection="host" is the default, has no selector, and an unknown value is refused at construction."""
    import inspect

    from step_amd import workloads

    assert inspect.signature(workloads.C4SelectTrainStep.__init__).parameters["selection"].default == "host"
    with pytest.raises(ValueError):
        workloads.C4SelectTrainStep(torch.device("cuda:0"), selection="gpu")


def _launch(args, prefix=(), env=None):
    r = subprocess.run([sys.executable] + list(prefix) + [os.path.join(ROOT, "train_step_amd.py"), "--iters", "3", "--warmup-iters", "2", "--log-every", "0"]
                       + list(args), capture_output=True, text=True, timeout=420, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    summ = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and json.loads(ln).get("summary")]
    assert len(summ) == 1, r.stdout[-2000:]
    return summ[0]


def test_train_step_amd_launcher_select_device_switch():
    """train_step_amd.py --select-device: exit 0, the summary says selection "device", the step is a hipGraph replay (one graph), and the
    generator ends at (warm-up + iterations) x 3 = 15 (dropout 0: only the selection draws)."""
    s = _launch(["--select-device"])
    assert s["selection"] == "device" and s["launch"] == "hipGraph replay (select-one)", s
    assert s["rng_offset"] == 15 and np.isfinite(s["final_loss"]) and s["final_loss"] > 0, s


def test_train_step_amd_launcher_select_device_without_graph():
    """--select-device --no-graph: no capture, and still the DEVICE selection (the padded eager iteration, not the ragged one, whose
    selection is the host's): the summary reports the selection that ran, the launch is eager, and the generator ends at (warm-up +
    iterations) x 3 = 15.  Plain --select --no-graph reports "host" and leaves the generator at 0."""
    s = _launch(["--select-device", "--no-graph"])
    assert s["selection"] == "device" and s["launch"] == "eager" and s["rng_offset"] == 15, s
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0, s
    s = _launch(["--select", "--no-graph"])
    assert s["selection"] == "host" and s["launch"] == "eager" and s["rng_offset"] == 0, s


def test_train_step_amd_launcher_select_device_two_ranks():
    """--select-device with a process group of two ranks (RCCL on two GPUs; on a one-GPU box the ranks share the GPU over gloo): the
    "select-one-split" form -- one graph from the first launch to the end of backward with the selection inside, ONE eager flat
    all-reduce, the update graph.  Finite loss, warm-up + iterations optimizer steps, 15 selection offsets on rank 0."""
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    two = torch.cuda.device_count() >= 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    s = _launch(["--select-device"] + ([] if two else ["--backend", "gloo"]),
                prefix=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port)], env=env)
    assert s["world_size"] == 2 and s["selection"] == "device" and s["launch"] == "hipGraph replay (select-one-split)", s
    assert s["adam_steps"] == 5 and s["rng_offset"] == 15 and s["gradient_exchange"] is not None, s
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0, s
