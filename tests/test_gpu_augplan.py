"""The device-drawn clip augmentation on the real gfx950 library: the cases of tests/augplan_cases.py (shared with the interpreter run of
tests/test_emul_augplan.py) plus what only exists on the device -- planner, fill and augment replayed in a graph, the absence of host
synchronisation, the training iteration whose selection reads the boxes the planner wrote, and the launcher's --augment-device switch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import augplan_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", PC.KERNEL_CASES)
def test_gpu_augplan_kernel(name, bk):
    PC.run_kernel_case(name, bk)


@pytest.mark.parametrize("name", PC.MODULE_CASES)
def test_gpu_augplan_module(name):
    getattr(PC, name)("cuda")


def _module(seed, offset):
    import step_amd

    gt, cnt, clips, d_gt, d_cnt = PC.module_inputs("cuda")
    rng = step_amd.DeviceRNG("cuda", seed=seed)
    rng.set_state((seed, offset))
    aug = step_amd.DeviceTubeAugmentation((PC.WN, PC.HN), PC.MEAN, PC.STDS, True, True, True, True, scale=PC.SCALE, rng=rng)
    bufs = (torch.empty((3, PC.T, 3, PC.HN, PC.WN), dtype=torch.float32, device="cuda"), torch.empty_like(d_gt), torch.empty_like(d_cnt))
    return aug, rng, gt, cnt, clips, d_gt, d_cnt, bufs


def test_replayed_graph_draws_anew():
    """planner + fill + augment captured in ONE graph and replayed three times: three different blocks, equal to the restatement at
    offsets o, o + 2, o + 4 (the recording itself draws nothing), pixels and ground truths with them"""
    seed, o = 33, 0xFFFF_FFFD                                                  # (the offset crosses 2^32 on the way)
    aug, rng, gt, cnt, clips, d_gt, d_cnt, bufs = _module(seed, o)
    aug.apply(clips, d_gt, d_cnt, out=bufs[0], gt_out=bufs[1], gt_count_out=bufs[2])          # builds the static block: not inside a capture
    rng.set_state((seed, o))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        aug.apply(clips, d_gt, d_cnt, out=bufs[0], gt_out=bufs[1], gt_count_out=bufs[2])
    assert rng.get_state() == (seed, o)
    blocks = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        PC.check_apply(aug, bufs, seed, o + 2 * k, PC._frames(), gt, cnt)
        blocks.append(aug.last_block().cpu().numpy().copy())
        assert rng.get_state() == (seed, o + 2 * k + 2)
    head = 4 * PC.layout(3, PC.GMAX, PC.MAX_HW)["patch_base"]
    assert not np.array_equal(blocks[0][:head], blocks[1][:head]) and not np.array_equal(blocks[1][:head], blocks[2][:head])


def test_apply_makes_no_host_synchronisation():
    """torch.cuda.set_sync_debug_mode("warn") reports every synchronising call: a warmed apply() makes NONE (no copy at all: the block, the
    frame addresses and the generator are resident)"""
    import warnings

    def reports(fn):
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode("default")
        return [str(x.message) for x in w if "synchronizing" in str(x.message) and "prototype" not in str(x.message)]

    x = torch.ones(8, device="cuda")
    assert len(reports(lambda: x.sum().item())) == 1 and len(reports(lambda: x + 1)) == 0        # the mode does report on this build
    aug, rng, gt, cnt, clips, d_gt, d_cnt, bufs = _module(5, 0)
    for _ in range(2):
        aug.apply(clips, d_gt, d_cnt, out=bufs[0], gt_out=bufs[1], gt_count_out=bufs[2])
    r = reports(lambda: [aug.apply(clips, d_gt, d_cnt, out=bufs[0], gt_out=bufs[1], gt_count_out=bufs[2]) for _ in range(4)])
    print("synchronising calls reported for apply():", len(r))
    assert r == []
    assert rng.get_state() == (5, 12)


SRC = (48, 64)


def _run(mode, steps=4, warm=2):
    import step_amd
    from step_amd import workloads

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    aug = step_amd.DeviceTubeAugmentation((400, 400), do_flip=True, do_crop=True, do_photometric=True, do_erase=True, scale=2)
    w = workloads.C4SelectTrainStep(dev, batch=1, seed=123, dtype=torch.bfloat16, capturable=(mode == "graph"), rng_seed=9, selection="device",
                                    augment=aug, src_size=SRC)
    assert aug.rng is w.rng and w.rng.get_state() == (9, 0) and w.selector.dynamic_gt
    with pytest.raises(RuntimeError):
        w.step()                                                               # the ragged form selects on the host: no augmentation there
    a, mid = w.args, int(w.args.NUM_CHUNKS[w.args.max_iter] / 2)
    losses, seen = [], []

    def note(loss):
        torch.cuda.synchronize()
        losses.append(float(loss))
        gt_out, cnt = w.d_gt.cpu().numpy(), w.d_gt_count.cpu().numpy()
        counts = w.select_counts()
        assert 1 <= cnt[0] <= 2 and not gt_out[0, cnt[0]:].any()
        rows = [r.tobytes() for r in gt_out[0, :cnt[0], mid, :4]]
        n_pos = 0
        for i in range(a.max_iter):
            pos = int(counts[i, 0, 0])
            assert 0 < pos <= a.max_pos_num and 0 <= counts[i, 0, 1] <= pos * a.neg_ratio
            tgt = w.s_tgt[i].cpu().numpy()
            for k in range(pos):                                               # clip 0's positives come first in its slots
                assert tgt[k, 1, 4] == 1 and tgt[k, 1, :4].tobytes() in rows, (i, k, tgt[k, 1, :4], gt_out[0, :cnt[0], mid, :4])
            n_pos += pos
        seen.append((gt_out.copy(), cnt.copy(), n_pos))

    if mode == "graph":
        w.capture(warmup=warm)
        assert w.graph_mode == "select-one" and w._gB is None
        assert w.rng.offset() == warm * (2 + 3)                                # the recording itself draws nothing
        for _ in range(steps - warm):
            note(w.step())
    else:
        for i in range(steps):
            loss = w.step_padded()
            if i >= warm:
                note(loss)
    out = (np.array(losses), w.rng.offset(), seen)
    del w
    torch.cuda.empty_cache()
    return out


def test_selection_trains_on_the_boxes_of_the_augmented_pixels():
    """C4SelectTrainStep(selection="device", augment=...), one clip, captured as ONE graph.  After each of two replays the boxes in the
    centre rows of the positives' targets are rows of THAT replay's gt_out (a middle-frame cache recorded outside the graph would hand the
    selection the boxes of an earlier iteration), the two replays' gt_out differ, a clip never gets positives without ground truths, every
    iteration uses 2 + 3 offsets, and the padded eager form gives the same losses bit for bit from the same state."""
    padded, graph = _run("padded"), _run("graph")
    assert padded[1] == graph[1] == 4 * (2 + 3)
    print("augment-device: losses padded %s graph %s, gt_count_out %s" % (padded[0].tolist(), graph[0].tolist(), [s[1].tolist() for s in graph[2]]))
    assert np.isfinite(graph[0]).all() and np.array_equal(padded[0], graph[0]), (padded[0], graph[0])
    (g0, c0, p0), (g1, c1, p1) = graph[2]
    assert not np.array_equal(g0, g1), "two replays wrote the same ground truths: the planner's offset did not advance in the graph"
    for (ga, ca, _), (gb, cb, _) in zip(padded[2], graph[2]):
        assert np.array_equal(ga, gb) and np.array_equal(ca, cb)


def test_workload_refuses_augment_with_host_selection():
    import step_amd
    from step_amd import workloads

    with pytest.raises(ValueError):
        workloads.C4SelectTrainStep(torch.device("cuda:0"), selection="host", augment=step_amd.DeviceTubeAugmentation((400, 400)))


def _child(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train_step_amd.py")] + list(args), capture_output=True, text=True, timeout=420, cwd=ROOT)


def test_launcher_augment_device():
    """train_step_amd.py --feed u8 --augment-device --select-device --iters 4 as a child process: the summary's feed reads
    u8+augment-device, gt_kept is the last iteration's kept tubes (1 or 2 of the clip's 2), and the generator ends at (3 warm-up + 4
    iterations) x (2 augmentation + 3 selection) offsets; with --dropout it would be 9 more per iteration (tests/test_gpu_select.py counts
    those).  Without its prerequisites the switch is refused with a message, before any device is touched."""
    r = _child(["--feed", "u8", "--augment-device", "--select-device", "--iters", "4", "--log-every", "0"])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    summ = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{") and json.loads(ln).get("summary")]
    assert len(summ) == 1, r.stdout[-2000:]
    s = summ[0]
    assert s["feed"] == "u8+augment-device" and s["selection"] == "device" and s["launch"] == "hipGraph replay (select-one)", s
    assert s["rng_offset"] == (3 + 4) * (2 + 3) and 1 <= s["gt_kept"] <= 2 and np.isfinite(s["final_loss"]) and s["final_loss"] > 0, s
    for bad in (["--augment-device"], ["--feed", "u8", "--augment-device"], ["--augment-device", "--select-device"],
                ["--feed", "u8", "--augment-device", "--select-device", "--augment"]):
        r = _child(bad + ["--iters", "1"])
        assert r.returncode != 0 and "--augment-device needs --feed u8 --select-device" in r.stderr, (bad, r.stderr[-500:])
