"""The SGD-with-momentum path on the real gfx950 library: the cases of tests/sgd_cases.py (shared with the interpreter run of
tests/test_emul_sgd.py) plus what only exists on the device -- the C4-sized arena, the captured training step with FlatSGD and the
launcher's --optimizer switch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sgd_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", SC.KERNEL_CASES + SC.KERNEL_GPU_ONLY)
def test_gpu_sgd_kernel(name, bk, golden):
    getattr(SC, name)(bk, golden)


@pytest.mark.parametrize("name", SC.MODULE_CASES)
def test_gpu_sgd_module(name, golden):
    getattr(SC, name)("cuda", golden)


def test_captured_sgd_training_step_follows_the_eager_steps():
    """C4TrainStep(optimizer="sgd") captured in one HIP graph against the same steps launched eagerly, as
    tests/test_gpu_graph_step.py demands of Adam (same structure, same 1e-5 / 1e-6 bounds: parameter delta, losses, state arena =
    momentum_buffer); the device-side counter -- which for SGD also decides which step initialises the buffer -- reads warm-up + replays.
    The split form (forward / backward graph, update graph: what a process group gets) is held to the same bounds."""
    from step_amd import workloads
    from step_amd.optim import FlatSGD

    dev = torch.device("cuda:0")
    steps, warm = 5, 2
    runs = {}
    for mode in ("eager", "graph", "split"):
        torch.manual_seed(7)
        w = workloads.C4TrainStep(dev, batch=1, seed=123, dtype=torch.bfloat16, capturable=(mode != "eager"), optimizer="sgd")
        assert isinstance(w.opt, FlatSGD) and w.opt.param_groups[0]["momentum"] == 0.9 and w.opt.param_groups[0]["weight_decay"] == 1e-7
        p0 = w.opt.flat_param.clone()
        losses = []
        if mode != "eager":
            w.capture(warmup=warm, mode="one" if mode == "graph" else "split")      # runs `warm` eager steps, records one more
            assert w.opt.step_count == warm
            for _ in range(steps - warm):
                losses.append(float(w.step()))
            assert w.graph is not None and w.graph_mode == ("one" if mode == "graph" else "split") and w.opt.step_count == steps
        else:
            for i in range(steps):
                l = float(w.step())
                if i >= warm:
                    losses.append(l)
            assert w.opt.step_count == steps
        torch.cuda.synchronize()
        runs[mode] = ((w.opt.flat_param - p0).double().cpu().numpy(), np.array(losses), w.opt.momentum_buffer.double().cpu().numpy())
        del w
        torch.cuda.empty_cache()
    da, la, ma = runs["eager"]
    for mode in ("graph", "split"):
        db, lb, mb = runs[mode]
        assert np.isfinite(db).all() and np.abs(db).max() > 0   # the parameters moved
        assert np.isfinite(lb).all()
        rel = float(np.linalg.norm(da - db) / np.linalg.norm(da))
        em = float(np.linalg.norm(ma - mb) / np.linalg.norm(ma))
        print("captured sgd step (%s): parameter delta rel %.3e, momentum_buffer rel %.3e, identical %s, losses %s / %s"
              % (mode, rel, em, bool(np.array_equal(da, db)), la.tolist(), lb.tolist()))
        assert rel < 1e-5 and em < 1e-5, (mode, rel, em)
        assert np.all(np.abs(la - lb) <= 1e-6 * np.abs(la)), (mode, la, lb)
        assert len(set(np.round(lb, 10))) > 1                   # the replays really advance the weights


def _launch(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_step_amd.py"), "--iters", "3", "--warmup-iters", "2", "--log-every", "0"] + list(args),
                       capture_output=True, text=True, timeout=420, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    summ = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and json.loads(ln).get("summary")]
    assert len(summ) == 1, r.stdout[-2000:]
    return summ[0]


def test_train_step_amd_launcher_optimizer_switch():
    """train_step_amd.py as a single-process launch: --optimizer sgd replays the captured step with FlatSGD (optimizer, opt_steps =
    warm-up + iterations, finite positive loss, no adam_steps), also around the host's proposal selection (--select); --optimizer adam
    keeps the summary's adam_steps beside the new keys."""
    s = _launch("--optimizer", "sgd")
    assert s["optimizer"] == "sgd" and s["opt_steps"] == 5 and "adam_steps" not in s
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0 and s["launch"].startswith("hipGraph replay")
    s = _launch("--optimizer", "sgd", "--select", "--momentum", "0.8", "--weight-decay", "1e-6")
    assert s["optimizer"] == "sgd" and s["opt_steps"] == 5 and s["launch"] == "hipGraph replay (select)"
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0
    s = _launch("--optimizer", "adam")
    assert s["optimizer"] == "adam" and s["opt_steps"] == 5 and s["adam_steps"] == 5
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0
