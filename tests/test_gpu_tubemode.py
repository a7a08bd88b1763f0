"""Tube growth outside temporal_mode "predict" on the real gfx950 library: the cases of tests/tubemode_cases.py (shared with the interpreter
run of tests/test_emul_tubemode.py) plus what only exists on the device -- driver.inference with the kernel against its tensor-op
restatement, GraphedInference under "extrapolate", the training iteration as one graph and the launcher's --temporal-mode switch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import tubemode_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", TC.KERNEL_CASES)
def test_gpu_tubemode_kernel(name, bk, golden):
    getattr(TC, name)(bk, golden)


@pytest.mark.parametrize("name", TC.MODULE_CASES)
def test_gpu_tubemode_module(name, golden):
    getattr(TC, name)("cuda", golden)


@pytest.mark.parametrize("mode", ["extrapolate", "mean"])
def test_inference_modes_kernel_against_restatement(mode, golden):
    TC.case_inference_modes_kernel("cuda", golden, mode)


def test_graphed_inference_extrapolate(golden):
    TC.case_graphed_inference_extrapolate("cuda:0", golden)


def _run(mode, iters=2, warm=2):
    from step_amd import workloads

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    w = workloads.C4SelectTrainStep(dev, batch=1, seed=123, dtype=torch.bfloat16, capturable=(mode == "graph"), rng_seed=9, selection="device",
                                    temporal_mode="extrapolate")
    assert w.args.temporal_mode == "extrapolate" and sorted(w.selector._ungrown) == [3]
    losses = []
    if mode == "graph":
        w.capture(warmup=warm)
        assert w.graph_mode == "select-one" and w._gB is None
        for _ in range(iters):
            loss = w.step()
            torch.cuda.synchronize()
            losses.append(float(loss))
    else:
        for i in range(warm + iters):
            loss = w.step_padded()
            if i >= warm:
                torch.cuda.synchronize()
                losses.append(float(loss))
    assert w.selection_ran == "device"
    counts = w.select_counts()
    out = (np.array(losses), w.rng.offset(), counts)
    del w
    torch.cuda.empty_cache()
    return out


def test_training_iteration_extrapolate_is_one_graph():
    """C4SelectTrainStep(selection="device", temporal_mode="extrapolate"), one clip, bf16: captured as ONE graph; the padded eager form gives
    the same losses bit for bit over two iterations from the same state; the losses are finite; every step selected positives."""
    padded, graph = _run("padded"), _run("graph")
    print("temporal_mode extrapolate: losses padded %s graph %s, offsets %d / %d" % (padded[0].tolist(), graph[0].tolist(), padded[1], graph[1]))
    assert padded[1] == graph[1] == 4 * 3
    assert np.isfinite(graph[0]).all() and np.array_equal(padded[0], graph[0]), (padded[0], graph[0])
    assert (graph[2][:, :, 0] > 0).all() and np.array_equal(padded[2], graph[2])


def test_workload_refuses_unknown_temporal_mode():
    from step_amd import workloads

    with pytest.raises(ValueError):
        workloads.C4SelectTrainStep(torch.device("cuda:0"), temporal_mode="linear")


def test_launcher_temporal_mode():
    """train_step_amd.py --select-device --temporal-mode extrapolate --iters 2 as a child process exits 0 and reports the mode; without a
    selecting iteration the switch is refused before any device is touched."""
    run = lambda args: subprocess.run([sys.executable, os.path.join(ROOT, "train_step_amd.py")] + args, capture_output=True, text=True,
                                      timeout=420, cwd=ROOT)
    r = run(["--select-device", "--temporal-mode", "extrapolate", "--iters", "2", "--log-every", "0"])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    summ = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and json.loads(ln).get("summary")]
    assert len(summ) == 1, r.stdout[-2000:]
    s = summ[0]
    assert s["temporal_mode"] == "extrapolate" and s["selection"] == "device" and s["launch"] == "hipGraph replay (select-one)", s
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0, s
    r = run(["--temporal-mode", "mean", "--iters", "1"])
    assert r.returncode != 0 and "--temporal-mode needs --select" in r.stderr, r.stderr[-500:]
