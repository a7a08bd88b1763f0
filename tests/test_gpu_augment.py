"""The device-side clip augmentation on the real gfx950 library: the cases of tests/augment_cases.py (shared with the interpreter run of
tests/test_emul_augment.py) plus what only exists on the device -- the full-size batch against the numpy restatement, the count of
apply()'s host synchronisations, and the training launcher fed through the augmentation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import augment_cases as AC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", AC.KERNEL_CASES)
def test_gpu_augment_kernel(name, bk, golden):
    getattr(AC, name)(bk, golden)


@pytest.mark.parametrize("name", AC.MODULE_CASES)
def test_gpu_augment_module(name, golden):
    getattr(AC, name)("cuda", golden)


def full_size_batch(seed=2027, N=8, T=36, H=256, W=340):
    """8 clips x 36 frames of 256x340 with the reference's training switches all on (scripts/train_step.sh:55-58), seeded."""
    from step_amd import TubeAugmentation

    rs = np.random.RandomState(seed)
    aug = TubeAugmentation((400, 400), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), True, True, True, True, scale=2)
    clips, plans = [], []
    np.random.seed(seed)
    for n in range(N):
        base = rs.randint(0, 256, (1, H // 4 + 1, W // 4 + 1, 3)).astype(np.float32)             # blocky colour + noise, some flat areas
        fr = np.clip(np.repeat(np.repeat(base, 4, 1), 4, 2)[:, :H, :W] + rs.randint(-20, 21, (T, H, W, 3)), 0, 255).astype(np.uint8)
        fr[:, 40:60, 50:90] = fr[:, 40:60, 50:90, :1]                                              # grey
        fr[:, 100:110, 200:230] = 0                                                                # black
        k = 1 + n % 3
        c = rs.uniform(0.3, 0.7, (k, 2))
        half = rs.uniform(0.1, 0.28, (k, 2))
        tubes = np.tile(np.concatenate([c - half, c + half], 1)[:, None, :].astype(np.float32), (1, T, 1))
        plan, _, _ = aug.plan((T, H, W), tubes)
        clips.append(fr)
        plans.append(plan)
    return aug, clips, plans


def test_full_size_batch_is_bit_equal_to_the_numpy_restatement():
    """8 x 36 x 256x340 -> 400x400, all four switches on: the kernel's fp32 output == np_apply for EVERY element (np_apply is pinned to
    the reference's own output by the fixture, tests/test_emul_augment.py)."""
    aug, clips, plans = full_size_batch()
    got = aug.apply([torch.from_numpy(c).cuda() for c in clips], plans, dtype=torch.float32, rgb=True).cpu().numpy()
    taken = dict(crop=0, mirror=0, erase=0, rects=0, first=0, hue=0)
    for n, (c, p) in enumerate(zip(clips, plans)):
        want = AC.nchw(AC.np_apply(c, p, aug.size, aug.scale, aug.mean, aug.stds), True)
        bad = int((got[n].view(np.uint32) != want.view(np.uint32)).sum())
        print("clip %d: crop %s mirror %d rects %d photometric flags %#x -> %d of %d elements differ" % (
            n, p.crop, p.mirror, len(p.rects), p.flags(), bad, want.size))
        assert bad == 0, (n, bad, float(np.abs(got[n] - want).max()))
        taken["crop"] += p.crop != (0, 0, p.Ws, p.Hs)
        taken["mirror"] += p.mirror
        taken["erase"] += len(p.rects) > 0
        taken["first"] += p.contrast_first
        taken["hue"] += p.hue is not None
    print(taken)
    assert taken["crop"] >= 4 and 0 < taken["mirror"] < len(plans) and taken["erase"] >= 3 and taken["hue"] >= 3 and 0 < taken["first"] < len(plans)


def test_apply_makes_no_host_synchronisation():
    """torch.cuda.set_sync_debug_mode("warn") reports every synchronising call: a warmed apply() makes NONE (one pinned block, one
    non-blocking copy, one launch)."""
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
    aug, clips, plans = full_size_batch(N=2, T=4)
    dev = [torch.from_numpy(c).cuda() for c in clips]
    out = torch.empty((2, 4, 3, 400, 400), dtype=torch.bfloat16, device="cuda")
    for _ in range(3):
        first = aug.apply(dev, plans, out=out).clone()
    r = reports(lambda: [aug.apply(dev, plans, out=out) for _ in range(4)])                        # (back to back: the pinned ring never waits)
    print("synchronising calls reported for apply():", len(r))
    assert r == []
    assert torch.equal(out, first)


def test_launcher_trains_through_the_augmentation():
    """train_step_amd.py --feed u8 --augment as a child process under its own time limit: a few iterations, a finite loss."""
    cmd = [sys.executable, os.path.join(ROOT, "train_step_amd.py"), "--iters", "4", "--feed", "u8", "--augment", "--log-every", "2",
           "--warmup-iters", "2"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    summary = [l for l in lines if l.get("summary")]
    print(summary)
    assert len(summary) == 1 and summary[0]["feed"] == "u8+augment" and np.isfinite(summary[0]["final_loss"])
    assert all(np.isfinite(l["loss"]) for l in lines if "loss" in l)
