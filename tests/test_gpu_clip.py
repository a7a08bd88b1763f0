"""Gradient-norm clipping and the device learning-rate schedules on the real gfx950 library: the cases of tests/clip_cases.py (shared with
the interpreter run of tests/test_emul_clip.py) plus what only exists on the device -- the C4-sized arena, a captured clip + step +
schedule, and the C4 training step with both inside its graph."""
import numpy as np
import pytest
import torch

from tests import clip_cases as CC
from tests import sgd_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", CC.KERNEL_CASES + CC.KERNEL_GPU_ONLY)
def test_gpu_clip_kernel(name, bk, golden):
    getattr(CC, name)(bk, golden)


@pytest.mark.parametrize("name", CC.MODULE_CASES)
def test_gpu_clip_module(name, golden):
    getattr(CC, name)("cuda", golden)


def test_captured_clip_step_and_schedule_follow_the_eager_twin():
    """clip_grad_norm_ + step + scheduler.step() on the six-segment arena, captured in one HIP graph after two eager warm-up steps (which
    create the norm workspace), against an eager twin: over 6 replays -- fresh gradients copied into the static arena in between -- the
    parameters, the momentum buffer, the stats block, the per-tensor norms, the lr table and both counters follow the twin BIT FOR BIT."""
    import step_amd

    dev = torch.device("cuda:0")
    gold = CC.lr_golden()["cases"][0]
    warm, replays = 2, 6
    grads = CC._gradients(seed=41, steps=warm + replays)
    m = float(np.median([np.sqrt(np.sum((g.astype(np.float64) * CC.GRAD_SCALE) ** 2)) for g in grads]))
    twins = []
    for _ in range(2):
        _, ps = CC._params(dev)
        o = CC._make("sgd", ps, capturable=True, lrs=[1e-5, 5e-5, 1e-4, 1e-5, 5e-5, 1e-4])
        twins.append((o, step_amd.DeviceWarmupCosineLR(o, **gold["args"])))

    def one(o, sch):
        o.clip_grad_norm_(m, grad_scale=CC.GRAD_SCALE)
        o.step(grad_scale=CC.GRAD_SCALE)
        sch.step()

    (oe, se), (og, sg) = twins
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    for k in range(warm):
        for o, sch in twins:
            CC._load_grad(o, grads[k])
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            one(og, sg)
        torch.cuda.current_stream(dev).wait_stream(side)
        one(oe, se)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one(og, sg)                                              # recorded, not run
    torch.cuda.synchronize()
    assert og.step_count == warm and sg.last_epoch == warm
    clipped = 0
    for k in range(warm, warm + replays):
        for o, _ in twins:
            CC._load_grad(o, grads[k])
        graph.replay()
        one(oe, se)
        torch.cuda.synchronize()
        for name in ("flat_param", "flat_grad", "momentum_buffer", "grad_norm", "seg_grad_norm", "_seg_lr", "_step_dev"):
            assert torch.equal(getattr(og, name), getattr(oe, name)), (k, name)
        assert sg.last_epoch == se.last_epoch == k + 1 and og.step_count == k + 1
        clipped += int(float(og.grad_norm[1]) < 1.0)
    assert 0 < clipped < replays                                 # some replays clipped, some did not: the same graph


LR_SCHEDULE = dict(milestones=[3, 6], min_ratio=0.01, cycle_decay=0.5, warmup_iters=2, warmup_factor=0.1)


def test_captured_c4_step_with_clip_and_schedule_follows_the_eager_steps():
    """C4TrainStep(batch=1, tubes_per_clip=5, bf16, capturable, max_grad_norm, lr_schedule) captured in one HIP graph against the same
    steps launched eagerly, with the structure and the 1e-5 / 1e-6 bounds of tests/test_gpu_graph_step.py; the clip is active (max_grad_norm
    1e-3 is far below the norm of this workload's gradients), the schedule's counter and lr table and the gradient norm follow too."""
    import step_amd
    from step_amd import workloads

    dev = torch.device("cuda:0")
    steps, warm = 5, 2
    runs = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(7)
        w = workloads.C4TrainStep(dev, batch=1, tubes_per_clip=5, seed=123, dtype=torch.bfloat16, capturable=True, max_grad_norm=1e-3,
                                  lr_schedule=lambda opt: step_amd.DeviceWarmupCosineLR(opt, **LR_SCHEDULE))
        assert isinstance(w.sched, step_amd.DeviceWarmupCosineLR) and w.opt.lr_scheduler is w.sched
        p0 = w.opt.flat_param.clone()
        losses = []
        if mode == "graph":
            w.capture(warmup=warm)
            assert w.opt.step_count == warm and w.sched.last_epoch == warm
            for _ in range(steps - warm):
                losses.append(float(w.step()))
            assert w.graph is not None
        else:
            for i in range(steps):
                l = float(w.step())
                if i >= warm:
                    losses.append(l)
        torch.cuda.synchronize()
        assert w.opt.step_count == steps and w.sched.last_epoch == steps
        st = w.opt.grad_norm.cpu().numpy()
        assert np.isfinite(st[0]) and st[0] > 1e-3 and 0 < st[1] < 1 and st[2] == 0, st
        runs[mode] = ((w.opt.flat_param - p0).double().cpu().numpy(), np.array(losses), w.opt.exp_avg.double().cpu().numpy(), st,
                      w.opt._seg_lr.cpu().numpy())
        del w
        torch.cuda.empty_cache()
    (da, la, ma, sa, lra), (db, lb, mb, sb, lrb) = runs["eager"], runs["graph"]
    assert np.isfinite(db).all() and np.abs(db).max() > 0
    rel = float(np.linalg.norm(da - db) / np.linalg.norm(da))
    em = float(np.linalg.norm(ma - mb) / np.linalg.norm(ma))
    print("captured C4 step with clip + schedule: parameter delta rel %.3e, exp_avg rel %.3e, identical %s, grad_norm %s / %s"
          % (rel, em, bool(np.array_equal(da, db)), sa.tolist(), sb.tolist()))
    assert rel < 1e-5 and em < 1e-5, (rel, em)
    assert np.all(np.abs(la - lb) <= 1e-6 * np.abs(la)), (la, lb)
    assert abs(sa[0] - sb[0]) <= 1e-5 * sa[0]
    assert np.array_equal(lra, lrb) and len(set(lra.tolist())) == 1 and lra[0] != np.float32(1e-5)     # the schedule's lr, not the constructor's
    assert len(set(np.round(lb, 10))) > 1


def test_c4_step_with_huge_max_grad_norm_equals_the_unclipped_step():
    """max_grad_norm = 1e30: the norm pass runs, the coefficient is exactly 1 and the workload's trajectory equals the un-clipped one BIT FOR
    BIT (three eager steps, bf16)."""
    from step_amd import workloads

    dev = torch.device("cuda:0")
    out = []
    for m in (None, 1e30):
        torch.manual_seed(7)
        w = workloads.C4TrainStep(dev, batch=1, tubes_per_clip=5, seed=123, dtype=torch.bfloat16, max_grad_norm=m)
        losses = [float(w.step()) for _ in range(3)]
        torch.cuda.synchronize()
        if m is not None:
            st = w.opt.grad_norm.cpu().numpy()
            assert st[1] == 1.0 and st[2] == 0.0 and np.isfinite(st[0]) and st[0] > 0
        else:
            assert w.opt.grad_norm is None
        out.append((w.opt.flat_param.clone(), w.opt.exp_avg.clone(), losses))
        del w
        torch.cuda.empty_cache()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
