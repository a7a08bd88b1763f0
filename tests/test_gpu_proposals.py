"""Detector proposals on the device path, on the real gfx950 library: the cases of tests/proposal_cases.py (shared with the interpreter
run of tests/test_emul_proposals.py) plus what only exists on the device -- the planner with tubes replayed in a graph, GraphedInference
over padded slots (one capture, any list of tubes), the training iteration that starts from proposals, and the launcher's --proposals."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from tests import augplan_cases as PC
from tests import proposal_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", RC.KERNEL_CASES)
def test_gpu_proposals_kernel(name, bk):
    RC.run_kernel_case(name, bk)


@pytest.mark.parametrize("name", RC.MODULE_CASES)
def test_gpu_proposals_module(name):
    getattr(RC, name)("cuda")


def test_apply_tubes_replayed_in_a_graph():
    """apply(tubes=...) on clips 0 and 1 (the two with ground truths: the host rule has an answer at every state) captured in ONE graph
    and replayed three times: tubes_out / tube_count_out equal the host rule's answer at offsets o, o + 2, o + 4 -- three different
    results, the recording itself draws nothing"""
    import step_amd

    seed, o = RC.GRAPH_STATE                                                    # (three usable offsets in a row, three different decisions)
    recs = [RC.restated(RC.ALL, seed, o + 2 * k) for k in range(3)]
    assert len({(r[4][1]["crop"], r[4][1]["mirror"]) for r in recs}) == 3
    (clips, d_gt, d_cnt, d_props, d_pcnt, d_fill), (props, counts) = RC.apply_inputs("cuda", clips=(0, 1))
    rng = step_amd.DeviceRNG("cuda", seed=seed)
    aug = step_amd.DeviceTubeAugmentation((PC.WN, PC.HN), PC.MEAN, PC.STDS, True, True, True, True, scale=PC.SCALE, rng=rng)
    bufs = dict(out=torch.empty((2, PC.T, 3, PC.HN, PC.WN), dtype=torch.float32, device="cuda"), gt_out=torch.empty_like(d_gt),
                gt_count_out=torch.empty_like(d_cnt), tubes_out=torch.empty_like(d_props), tube_count_out=torch.empty_like(d_pcnt))
    aug.apply(clips, d_gt, d_cnt, tubes=d_props, tube_count=d_pcnt, fill=d_fill, **bufs)      # builds the static block: not inside a capture
    rng.set_state((seed, o))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        aug.apply(clips, d_gt, d_cnt, tubes=d_props, tube_count=d_pcnt, fill=d_fill, **bufs)
    assert rng.get_state() == (seed, o)
    seen = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        exp = RC.expected_tubes(RC.ALL, seed, o + 2 * k, props, counts, RC.FILL, clips=(0, 1))
        got = bufs["tubes_out"].cpu().numpy()
        assert np.array_equal(got.view(np.int32), exp[0].view(np.int32)) and np.array_equal(bufs["tube_count_out"].cpu().numpy(), exp[1]), k
        assert rng.get_state() == (seed, o + 2 * k + 2)
        seen.append(got.copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[2])


def _reports(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return [str(x.message) for x in w if "synchronizing" in str(x.message) and "prototype" not in str(x.message)]


def test_graphed_inference_with_a_capacity():
    """GraphedInference(capacity=4), B = 2, fp32: ONE capture replayed with lists of (3, 1), (0, 4) and (4, 4) tubes.  Each replay equals
    the eager inference_flat on the same padded buffers bit for bit; its real rows agree with the ragged driver.inference on the same lists
    within the bound tests/module_cases.py holds these tensors to against the golden history (rel < 1e-3; whether they are bit-equal is
    printed).  Five tubes in a clip raise, and a warmed call reports no host synchronisation."""
    from step_amd import driver, workloads
    from tests.module_cases import np_, rel

    dev = torch.device("cuda:0")
    w = workloads.C3Inference(dev, torch.float32, batch=2, tubes=4, graph=False)
    rs = np.random.RandomState(3)

    def lists(ns):
        out = []
        for n in ns:
            xy = rs.uniform(10, 250, (n, 1, 2))
            box = np.concatenate([xy, xy + rs.uniform(60, 140, (n, 1, 2))], 2)
            out.append((box + rs.uniform(-4, 4, (n, 3, 4))).astype(np.float32))
        return out

    gi = driver.GraphedInference(w.args, w.base, w.ctx, w.nets, w.x, lists((3, 1)), capacity=4)
    graph = gi.graph
    clip_of = torch.arange(2, device=dev).repeat_interleave(4)
    keys = ("pred_prob", "pred_loc", "pred_first_loc", "pred_last_loc")
    with torch.no_grad():
        cf = w.base(w.x)
        cx = w.ctx(cf)
        for ns in ((3, 1), (0, 4), (4, 4)):
            tl = lists(ns)
            hist, _, _ = gi(None, tl)
            torch.cuda.synchronize()
            assert gi.graph is graph and gi.count.tolist() == list(ns)
            assert all(h["tubes_count"] is gi.count and h["tubes_nums"] == [4, 4] for h in hist)
            flat, count = driver.pad_tubes(tl, 4, dev, 400, 400)
            assert torch.equal(gi.flat0, flat) and torch.equal(gi.count, count)
            eager, _ = driver.inference_flat(w.args, cf, cx, w.nets, 3, flat, [4, 4], clip_of, want_classes=False, counts=count)
            for i, (a, b) in enumerate(zip(hist, eager)):
                for k in keys:
                    assert torch.equal(a[k], b[k]), (ns, i, k)
            ragged, _ = driver.inference(w.args, cf, cx, w.nets, 3, tl)
            real = torch.tensor([s < ns[b] for b in range(2) for s in range(4)], device=dev)
            same = True
            for i, (a, b) in enumerate(zip(hist, ragged)):
                for k in keys:
                    e = rel(np_(a[k][real]), np_(b[k]))
                    same = same and torch.equal(a[k][real], b[k])
                    assert e < 1e-3, (ns, i, k, e)
            print("padded replay vs ragged inference at %s tubes: bit-equal %s" % (ns, same))
        with pytest.raises(ValueError):
            gi(None, lists((5, 1)))
        tl = lists((2, 3))
        for _ in range(3):
            gi(None, tl)
        r = _reports(lambda: [gi(None, tl) for _ in range(4)])
        print("synchronising calls reported for GraphedInference(capacity=4):", len(r))
        assert r == []


SRC = (48, 64)
K = 8


def _train(mode, steps=4, warm=2):
    import step_amd
    from step_amd import workloads

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    aug = step_amd.DeviceTubeAugmentation((400, 400), do_flip=True, do_crop=True, do_photometric=True, do_erase=True, scale=2)
    w = workloads.C4SelectTrainStep(dev, batch=2, seed=123, dtype=torch.bfloat16, capturable=True, rng_seed=9, selection="device", augment=aug,
                                    src_size=SRC, proposals=K)
    assert w.d_prop_count.tolist()[1] == 0 and 1 <= w.d_prop_count.tolist()[0] <= K        # the second clip falls back to the fill
    a = w.args
    losses, counts = [], []

    def note(loss):
        torch.cuda.synchronize()
        losses.append(float(loss))
        cnt = w.d_count.cpu().numpy()
        assert cnt[1] == min(34, K) and cnt[0] == w.d_prop_count.tolist()[0]
        cand = w.d_init.view(2, K, 3, 4).cpu().numpy()
        whole = np.array([0, 0, 400, 400], np.float32)
        sel, mask = w.s_flat[0].cpu().numpy(), w.s_mask[0].cpu().numpy()
        picked = 0
        for b in range(2):
            assert np.all(cand[b, cnt[b]:] == whole)
            rows = {cand[b, s].tobytes() for s in range(cnt[b])}
            for r in range(w.budget):
                o = b * w.budget + r
                if mask[o, 0] == 1:
                    assert sel[o, :, 1:].tobytes() in rows, (b, r, sel[o, :, 1:])
                    picked += 1
        sc = w.select_counts()
        assert picked == int(sc[0].sum()) and np.all(sc.sum(axis=2) <= cnt[None, :])
        counts.append(sc.copy())

    if mode == "graph":
        w.capture(warmup=warm)
        assert w.graph_mode == "select-one" and w._gB is None
        for _ in range(steps - warm):
            note(w.step())
    else:
        for i in range(steps):
            loss = w.step_padded()
            if i >= warm:
                note(loss)
    params = torch.cat([p.detach().float().flatten() for p in w.params]).cpu().numpy()
    return w, np.array(losses), params, counts


def test_training_iteration_from_proposals():
    """C4SelectTrainStep(selection="device", proposals=8, augment=all four switches), two clips, bf16: capture() plus two replays give the
    parameters and losses of step_padded() calls from the same state bit for bit.  After each iteration every step-1 selected row with
    mask 1 is one of its clip's first `count` transformed proposals -- never a padded slot -- and no step selects more rows than the clip
    has real tubes.  set_proposals between replays changes the counts the selection can reach, without a recapture."""
    wp, lp, pp, cp = _train("padded")
    del wp
    torch.cuda.empty_cache()
    w, lg, pg, cg = _train("graph")
    print("proposals: losses padded %s graph %s, selected %s" % (lp.tolist(), lg.tolist(), [c.sum(axis=2).tolist() for c in cg]))
    assert np.isfinite(lg).all() and np.array_equal(lp, lg), (lp, lg)
    assert np.array_equal(pp, pg)
    assert all(np.array_equal(a, b) for a, b in zip(cp, cg))
    graph = w._gF
    rs = np.random.RandomState(1)

    def props(n):
        xy = rs.uniform(0.05, 0.5, (n, 1, 2))
        return np.concatenate([xy, xy + rs.uniform(0.2, 0.4, (n, 1, 2))], 2).repeat(3, axis=1).astype(np.float32)

    w.set_proposals([props(1), props(1)])
    w.step()
    torch.cuda.synchronize()
    assert w._gF is graph and w.d_count.tolist() == [1, 1]
    assert np.all(w.select_counts().sum(axis=2) <= 1)
    w.set_proposals([props(K), props(0)])
    w.step()
    torch.cuda.synchronize()
    assert w._gF is graph and w.d_count.tolist() == [K, min(34, K)] and np.isfinite(float(w.loss))
    with pytest.raises(ValueError):
        w.set_proposals([props(K + 1), props(0)])


def test_proposals_without_augmentation():
    """proposals=8 without augment=: the proposals are scaled once at construction (the clip without any holds the fill), step_padded()
    selects among the real slots only, and the ragged step() runs the host selection on the real ragged lists; set_proposals rewrites
    the slots themselves"""
    from step_amd import workloads

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    w = workloads.C4SelectTrainStep(dev, batch=2, seed=123, dtype=torch.bfloat16, rng_seed=9, selection="device", proposals=K)
    cnt = w.d_count.tolist()
    assert cnt == [len(t) for t in w.init_tubes] and cnt[1] == min(34, K) and 1 <= cnt[0] <= K
    slots = w.flat0[:, :, 1:].view(2, K, 3, 4).cpu().numpy()
    for b in range(2):
        assert np.array_equal(slots[b, :cnt[b]], w.init_tubes[b]) and np.all(slots[b, cnt[b]:] == np.array([0, 0, 400, 400], np.float32))
    assert np.array_equal(w.init_tubes[1], np.repeat((w.fill * 400.0).astype(np.float32)[:, None, :], 3, axis=1))
    loss = float(w.step_padded())
    torch.cuda.synchronize()
    assert np.isfinite(loss) and w.selection_ran == "device"
    sel, mask = w.s_flat[0].cpu().numpy(), w.s_mask[0].cpu().numpy()
    for b in range(2):
        rows = {slots[b, s].tobytes() for s in range(cnt[b])}
        assert all(sel[b * w.budget + r, :, 1:].tobytes() in rows for r in range(w.budget) if mask[b * w.budget + r, 0] == 1)
    assert np.all(w.select_counts().sum(axis=2) <= np.array(cnt)[None, :]) and w.select_counts()[0].sum() > 0
    loss = float(w.step())                                                     # the ragged form: host selection on the real lists
    assert np.isfinite(loss) and w.selection_ran == "host" and all(n <= c for n, c in zip(w.selected[0], cnt))
    one = np.tile(np.array([[0.2, 0.2, 0.6, 0.7]], np.float32), (1, 3, 1))
    w.set_proposals([one, one])
    assert w.d_count.tolist() == [1, 1] and np.array_equal(w.d_init[0].cpu().numpy(), w.init_tubes[0][0])
    assert np.isfinite(float(w.step_padded())) and np.all(w.select_counts().sum(axis=2) <= 1)


def test_workload_refuses_proposals_with_host_selection():
    from step_amd import workloads

    with pytest.raises(ValueError):
        workloads.C4SelectTrainStep(torch.device("cuda:0"), selection="host", proposals=8)


def _child(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "train_step_amd.py")] + list(args), capture_output=True, text=True, timeout=420, cwd=ROOT)


def test_launcher_proposals():
    """train_step_amd.py --select --select-device --feed u8 --augment-device --proposals 8 --iters 3 as a child process: finite losses and
    "proposals": 8 in the summary; without --select-device the switch is refused with a message before any device is touched."""
    r = _child(["--select", "--select-device", "--feed", "u8", "--augment-device", "--proposals", "8", "--iters", "3", "--log-every", "1"])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    summ = [ln for ln in lines if ln.get("summary")]
    assert len(summ) == 1, r.stdout[-2000:]
    s = summ[0]
    assert s["proposals"] == 8 and 1 <= s["proposals_real"] <= 8 and s["selection"] == "device" and s["feed"] == "u8+augment-device", s
    assert np.isfinite(s["final_loss"]) and s["final_loss"] > 0, s
    losses = [ln["loss"] for ln in lines if "loss" in ln and not ln.get("summary")]
    assert len(losses) >= 3 and np.isfinite(losses).all(), losses
    r = _child(["--select", "--proposals", "8", "--iters", "1"])
    assert r.returncode != 0 and "--proposals K needs --select-device" in r.stderr, r.stderr[-500:]
