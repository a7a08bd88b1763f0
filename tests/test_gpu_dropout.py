"""The device-side dropout on the real gfx950 library: the cases of tests/dropout_cases.py (shared with the interpreter run of
tests/test_emul_dropout.py) plus what only exists on the device -- one full-size call site, the captured C4 step at the reference's
dropout = 0.3 in its three launch forms, the captured selection step and the launcher's --dropout switch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dropout_cases as DC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", DC.KERNEL_CASES + DC.KERNEL_GPU_ONLY)
def test_gpu_dropout_kernel(name, bk, golden):
    getattr(DC, name)(bk, golden)


@pytest.mark.parametrize("name", DC.MODULE_CASES)
def test_gpu_dropout_module(name, golden):
    getattr(DC, name)("cuda", golden)


def _run_c4(mode, dropout, steps=5, warm=2, rng_seed=31):
    from step_amd import workloads

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    w = workloads.C4TrainStep(dev, batch=1, seed=123, dtype=torch.bfloat16, capturable=(mode != "eager"), optimizer="adam", dropout=dropout,
                              rng_seed=rng_seed)
    assert w.rng.get_state() == (rng_seed, 0)
    p0 = w.opt.flat_param.clone()
    losses = []
    if mode != "eager":
        w.capture(warmup=warm, mode="one" if mode == "graph" else "split")          # runs `warm` eager steps, records one more
        after_capture = w.rng.offset()
        for _ in range(steps - warm):
            losses.append(float(w.step()))
        assert w.graph is not None and w.opt.step_count == steps
    else:
        after_capture = None
        for i in range(steps):
            l = float(w.step())
            if i >= warm:
                losses.append(l)
    torch.cuda.synchronize()
    out = ((w.opt.flat_param - p0).double().cpu().numpy(), np.array(losses),
           torch.cat([w.opt.exp_avg, w.opt.exp_avg_sq]).double().cpu().numpy(), w.rng.offset(), after_capture)
    del w
    torch.cuda.empty_cache()
    return out


def test_captured_dropout_training_step_follows_the_eager_steps():
    """C4TrainStep(dropout=0.3, bf16, Adam) eager, as one HIP graph and in the split form: structure and bounds of
    test_captured_sgd_training_step_follows_the_eager_steps (parameter delta and state arena within 1e-5, losses within 1e-6 relative:
    the project's bounds for graph against eager) -- the replays draw the masks the eager steps draw, because a mask depends on (seed,
    offset, element) only and the offset advances on the device.  In addition: two graph runs from the same seed are bit-identical; the
    final offset is steps x 9 (3 heads x 3 sites) in all three forms, and the recording pass itself does not advance it (warm x 9 right
    after capture()); the losses differ from a dropout = 0 run."""
    steps, warm = 5, 2
    runs = {m: _run_c4(m, 0.3, steps, warm) for m in ("eager", "graph", "split")}
    again = _run_c4("graph", 0.3, steps, warm)
    plain = _run_c4("eager", 0.0, steps, warm)
    da, la, ma, off, _ = runs["eager"]
    assert off == steps * 9
    assert plain[3] == 0
    for mode in ("graph", "split"):
        db, lb, mb, offb, after = runs[mode]
        assert after == warm * 9, (mode, after)
        assert offb == steps * 9, (mode, offb)
        assert np.isfinite(db).all() and np.abs(db).max() > 0 and np.isfinite(lb).all()
        rel = float(np.linalg.norm(da - db) / np.linalg.norm(da))
        em = float(np.linalg.norm(ma - mb) / np.linalg.norm(ma))
        print("captured dropout step (%s): parameter delta rel %.3e, state rel %.3e, identical %s, losses %s / %s"
              % (mode, rel, em, bool(np.array_equal(da, db)), la.tolist(), lb.tolist()))
        assert rel < 1e-5 and em < 1e-5, (mode, rel, em)
        assert np.all(np.abs(la - lb) <= 1e-6 * np.abs(la)), (mode, la, lb)
        assert len(set(np.round(lb, 10))) > 1
    g1 = runs["graph"]
    assert np.array_equal(g1[0], again[0]) and np.array_equal(g1[1], again[1]) and np.array_equal(g1[2], again[2]) and again[3] == steps * 9
    assert not np.any(la == plain[1]), (la, plain[1])


def test_captured_select_step_with_dropout_is_bit_identical():
    """C4SelectTrainStep(dropout=0.3): step_padded() and capture() walk the same trajectory bit for bit, as tests/test_gpu_graph_step.py
    demands at dropout = 0 (same kernels on the same buffers, and the same masks: same seed, same offsets)."""
    import random

    from step_amd import workloads

    dev = torch.device("cuda:0")
    steps, warm = 4, 2
    out = {}
    for mode in ("padded", "graph"):
        random.seed(5)
        np.random.seed(5)
        torch.manual_seed(7)
        w = workloads.C4SelectTrainStep(dev, batch=1, seed=123, dtype=torch.bfloat16, capturable=(mode == "graph"), dropout=0.3, rng_seed=9)
        p0 = w.opt.flat_param.clone()
        losses = []
        if mode == "graph":
            w.capture(warmup=warm)
            for _ in range(steps - warm):
                losses.append(float(w.step()))
        else:
            for i in range(steps):
                l = float(w.step_padded())
                if i >= warm:
                    losses.append(l)
        torch.cuda.synchronize()
        out[mode] = ((w.opt.flat_param - p0).cpu().numpy(), np.array(losses), w.rng.offset(), w.opt.step_count)
        del w
        torch.cuda.empty_cache()
    a, b = out["padded"], out["graph"]
    assert a[2] == b[2] == steps * 9 and a[3] == b[3] == steps
    assert np.isfinite(b[1]).all() and np.abs(b[0]).max() > 0
    assert np.array_equal(a[1], b[1]), (a[1], b[1])
    assert np.array_equal(a[0], b[0])


def _launch(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_step_amd.py"), "--iters", "3", "--warmup-iters", "2", "--log-every", "0"] + list(args),
                       capture_output=True, text=True, timeout=420, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    summ = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and json.loads(ln).get("summary")]
    assert len(summ) == 1, r.stdout[-2000:]
    return summ[0]


def test_train_step_amd_launcher_dropout_switch():
    """train_step_amd.py --dropout 0.3: the captured step replays with the device-side dropout (summary: dropout, rng_offset = (warm-up
    + iterations) x 9 = 45, finite positive loss, a hipGraph replay launch); --dropout 0 leaves the generator at offset 0."""
    s = _launch("--dropout", "0.3")
    assert s["dropout"] == 0.3 and s["rng_offset"] == 45
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0 and s["launch"].startswith("hipGraph replay")
    s = _launch("--dropout", "0")
    assert s["dropout"] == 0 and s["rng_offset"] == 0 and s["launch"].startswith("hipGraph replay")
