"""The classification pre-training stage on the real gfx950 library: the cases of tests/cls_cases.py (shared with the interpreter run of
tests/test_emul_cls.py) plus what only exists on the device -- workloads.C4ClsTrainStep with the iteration as ONE captured graph, for the
host's and the device's sampling and selection, and the launcher's --cls switch."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cls_cases as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", CC.KERNEL_CASES)
def test_gpu_cls_kernel(name, bk, golden):
    getattr(CC, name)(bk, golden)


@pytest.mark.parametrize("name", CC.MODULE_CASES)
def test_gpu_cls_module(name, golden):
    getattr(CC, name)("cuda", golden)


def _run(mode, selection, dropout, steps=4, warm=2):
    from step_amd import workloads

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    random.seed(21)                                              # (the host's sampling and selection: the reference's two streams)
    np.random.seed(21)
    w = workloads.C4ClsTrainStep(dev, batch=2, seed=123, dtype=torch.bfloat16, capturable=(mode == "graph"), dropout=dropout, rng_seed=9,
                                 selection=selection)
    assert w.rng.get_state() == (9, 0)
    p0 = w.opt.flat_param.clone()
    losses, picks = [], []

    def note(loss):
        losses.append(float(loss))
        picks.append((w.s_flat.cpu().numpy().copy(), w.s_tgt.cpu().numpy().copy(), w.s_mask.cpu().numpy().copy(), list(w.selected)))
        assert w.selection_ran == selection

    if mode == "graph":
        w.capture(warmup=warm)
        assert w.graph_mode == "cls-one" and w.graph is not None and w._g_update is None
        per = (2 if selection == "device" else 0) + (2 if dropout else 0)
        assert w.rng.offset() == warm * per                                       # the recording itself draws nothing
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


@pytest.mark.parametrize("selection", ["host", "device"])
def test_cls_step_is_one_graph_and_bit_identical(selection):
    """C4ClsTrainStep(bf16, batch 2, dropout 0.3, rng_seed 9), 4 iterations of which 2 warm up: step_padded() and capture() give the same
    losses and the same parameter delta bit for bit (same kernels on the same buffers, same draws); the captured form is ONE graph
    ("cls-one", no update graph); two captured runs from one seed are identical.  Offsets per iteration, from the code: a cls_only head has
    TWO dropout sites (heads.TwoBranchNet.forward: the flattened feature and the context vector; the third site is in the local branch a
    cls_only head does not have) and the device selection makes TWO launches that own an offset (step_anchor_sample, step_select_train) --
    so the generator ends at 4 x (2 + 2) with selection="device" and at 4 x 2 with selection="host" (4 x 2 and 0 with dropout 0).  The
    device selection differs between two replays; the host selection follows `random` / `numpy.random` (seeded alike in every run)."""
    steps = 4
    padded, graph, again = _run("padded", selection, 0.3), _run("graph", selection, 0.3), _run("graph", selection, 0.3)
    plain = _run("padded", selection, 0.0)
    sel_off = 2 if selection == "device" else 0
    assert padded[2] == graph[2] == again[2] == steps * (sel_off + 2) and plain[2] == steps * sel_off
    assert padded[3] == graph[3] == steps
    assert np.isfinite(graph[1]).all() and np.isfinite(plain[1]).all() and np.abs(graph[0]).max() > 0
    print("cls %s selection: losses padded %s graph %s, rows per clip %s" % (selection, padded[1].tolist(), graph[1].tolist(), [p[3] for p in graph[4]]))
    assert np.array_equal(padded[1], graph[1]), (padded[1], graph[1])
    assert np.array_equal(padded[0], graph[0])
    assert np.array_equal(graph[0], again[0]) and np.array_equal(graph[1], again[1])
    for a, b in zip(padded[4], graph[4]):
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
        assert all(2 <= n <= 20 for n in a[3]) and a[2].sum() == sum(a[3])
    (f0, _, _, _), (f1, _, _, _) = graph[4]
    assert not np.array_equal(f0, f1), "two replays trained on the same boxes"


def test_cls_host_ragged_and_padded_select_the_same_rows():
    """selection="host": under the same `random` / `numpy.random` seeds the ragged step() and step_padded() sample and select the same
    rows -- the padded form's real slots are the ragged form's tubes and targets, clip by clip, with mask 1 on exactly those slots and
    inv = 1 / (rows x classes); both losses are printed (the head of the padded form sees the padded rows too, with weight 0)."""
    from step_amd import workloads

    dev = torch.device("cuda:0")
    got = {}
    for form in ("ragged", "padded"):
        random.seed(5)
        np.random.seed(5)
        w = workloads.C4ClsTrainStep(dev, batch=2, seed=123, dtype=torch.bfloat16, selection="host")
        loss = float(w.step() if form == "ragged" else w.step_padded())
        assert w.selection_ran == "host" and w.rng.offset() == 0
        sel, tgt = w.last_selection
        got[form] = (sel, tgt, loss, w.s_flat.cpu().numpy(), w.s_tgt.cpu().numpy(), w.s_mask.cpu().numpy(), float(w.s_inv.cpu()[0]))
        del w
        torch.cuda.empty_cache()
    (rs_, rt, rl, _, _, _, _), (ps, pt, pl, flat, tgt, mask, inv) = got["ragged"], got["padded"]
    rows = 0
    for b in range(2):
        assert np.array_equal(rs_[b], ps[b]) and np.array_equal(rt[b], pt[b])
        n = len(rs_[b])
        assert np.array_equal(flat[b * 20:b * 20 + n, :, 1:], rs_[b]) and np.array_equal(tgt[b * 20:b * 20 + n], rt[b])
        assert mask[b * 20:b * 20 + n].all() and not mask[b * 20 + n:(b + 1) * 20].any() and not tgt[b * 20 + n:(b + 1) * 20].any()
        rows += n
    assert inv == np.float32(1.0 / (rows * 60))
    print("cls ragged loss %.6f, padded loss %.6f" % (rl, pl))
    assert np.isfinite(rl) and np.isfinite(pl) and rl > 0 and pl > 0


def test_cls_host_selection_stays_the_default():
    import inspect

    from step_amd import workloads

    assert inspect.signature(workloads.C4ClsTrainStep.__init__).parameters["selection"].default == "host"
    with pytest.raises(ValueError):
        workloads.C4ClsTrainStep(torch.device("cuda:0"), selection="gpu")


def _launch(args, prefix=(), env=None):
    r = subprocess.run([sys.executable] + list(prefix) + [os.path.join(ROOT, "train_step_amd.py"), "--iters", "3", "--warmup-iters", "2", "--log-every", "0"]
                       + list(args), capture_output=True, text=True, timeout=420, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    summ = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and json.loads(ln).get("summary")]
    assert len(summ) == 1, r.stdout[-2000:]
    return summ[0]


@pytest.mark.parametrize("flags,selection,launch,offset", [
    (["--cls"], "host", "hipGraph replay (cls-one)", 0),
    (["--cls", "--select-device"], "device", "hipGraph replay (cls-one)", 10),
    (["--cls", "--select-device", "--no-graph"], "device", "eager", 10)])
def test_train_step_amd_launcher_cls(flags, selection, launch, offset):
    """train_step_amd.py --cls (one fresh process each): exit 0, the summary names the workload, the selection that ran and the launch --
    one replayed graph, or eager with --no-graph -- and the generator ends at (warm-up + iterations) x 2 = 10 with the device selection
    (dropout 0: only step_anchor_sample and step_select_train draw) and at 0 with the host's."""
    s = _launch(flags)
    assert s["workload"] == "cls" and s["selection"] == selection and s["launch"] == launch and s["rng_offset"] == offset, s
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0 and s["opt_steps"] == 5, s


def test_train_step_amd_launcher_cls_two_ranks():
    """--cls --select-device with a process group of two ranks (RCCL on two GPUs; on a one-GPU box the ranks share the GPU over gloo): the
    split form -- one graph from the first launch to the end of backward with sampling and selection inside, ONE eager flat all-reduce, the
    update graph.  Finite loss, warm-up + iterations optimizer steps, 10 selection offsets on rank 0."""
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    two = torch.cuda.device_count() >= 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    s = _launch(["--cls", "--select-device"] + ([] if two else ["--backend", "gloo"]),
                prefix=["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port)], env=env)
    assert s["world_size"] == 2 and s["workload"] == "cls" and s["selection"] == "device" and s["launch"] == "hipGraph replay (cls-split)", s
    assert s["adam_steps"] == 5 and s["rng_offset"] == 10 and s["gradient_exchange"] is not None, s
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0, s
