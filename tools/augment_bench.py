"""step_clip_augment_u8 at the training shape -- 8 clips x 36 frames, 256x340 -> 400x400, bf16 -- ONE process, every launch timed between
device events after a warm-up, the forms alternated round by round, the spread (min .. max of the rounds) reported beside the median:

  * the kernel under three plans: BaseTransform only (resize), geometry only (crop + mirror + erase + resize), all four switches;
  * step_clip_from_u8 at [8,36,400,400] in the same process (it writes the same bytes and reads 1.6x as many);
  * for each, the bytes the algorithm needs (source frames once + output once + erase patches) over that time, as a share of what
    step_hbm_stream_probe moves on the same box in the same process;
  * host time of `.plan` per clip, and of the numpy restatement `tests/augment_cases.np_apply` per clip -- a CPU time on this box's
    host, the stand-in for what the reference's loader pays per clip in numpy / OpenCV (the reference's own transform needs cv2, which
    is not installed here);
  * --train-runs K: train_step_amd.py --feed u8 against --feed u8 --augment as child processes, alternated, K runs each.

--device-plan runs another leg INSTEAD: the decisions of the same batch made on the device (step_augment_plan: planner + noise fill, timed
between device events) beside the host form (`.plan` per clip + pack + the copy of the block, wall time up to the copy's completion), rounds
alternated; and with --train-runs K, train_step_amd.py --feed u8 --augment --select-device against --feed u8 --augment-device
--select-device at 1 and 8 clips per GPU, child processes alternated, K runs each, each form's own spread beside its median.  With
--plan-tubes P the leg also times planner + fill WITH P proposals per clip (step_augment_plan_tubes) against the same call without tubes,
at 1 and 8 clips, rounds alternated.

    python tools/augment_bench.py [--out profiles/clip_augment_timing.txt] [--train-runs 3]
    python tools/augment_bench.py --device-plan --train-runs 3 --out profiles/augment_plan_timing.txt
    python tools/augment_bench.py --device-plan --plan-tubes 34
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from step_amd import BaseTransform, TubeAugmentation, _capi, _lib, ops
from tools import abkit

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--launches", type=int, default=50, help="timed launches per form and round")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--train-runs", type=int, default=0)
ap.add_argument("--train-iters", type=int, default=60)
ap.add_argument("--np-clips", type=int, default=2, help="clips the numpy restatement is timed on")
ap.add_argument("--device-plan", action="store_true", help="the step_augment_plan leg instead of the kernel forms (see above)")
ap.add_argument("--plan-tubes", type=int, default=0, metavar="P", help="--device-plan: also time the planner with P proposals per clip")
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/augment_bench.py needs a ROCm device"
dev = torch.device("cuda:0")
L = _lib.lib()
say = abkit.tee(a.out)
timed = abkit.event_ms                                                         # ms per launch, no warm-up of its own: every form is warmed below

N, T, Hs, Ws, Ho, Wo = 8, 36, 256, 340, 400, 400
rs = np.random.RandomState(11)
frames_np = rs.randint(0, 256, (N, T, Hs, Ws, 3)).astype(np.uint8)
frames = torch.from_numpy(frames_np).to(dev)
centre, half = rs.uniform(0.35, 0.65, (N, 2, 1, 2)), rs.uniform(0.1, 0.25, (N, 2, 1, 2))
tubes = np.tile(np.concatenate([centre - half, centre + half], 3), (1, 1, T, 1)).astype(np.float32)
out = torch.empty((N, T, 3, Ho, Wo), dtype=torch.bfloat16, device=dev)


def train_children(forms, extra, what):
    """the launcher as child processes, the forms alternated run by run -> {form: [ms per iteration]}"""
    runs = {f: [] for f in forms}
    for r in range(a.train_runs):
        for form in runs:
            cmd = [sys.executable, os.path.join(ROOT, "train_step_amd.py"), "--iters", str(a.train_iters), "--log-every", "0"] + form.split() + extra
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                say("train_step_amd.py %s failed (%d): %s" % (form, p.returncode, (p.stdout + p.stderr)[-800:]))
                raise SystemExit(1)                                            # (nothing more is started after a failed child)
            s = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{") and "summary" in l][-1]
            runs[form].append(s["ms_per_iter"])
    say("train_step_amd.py, %s, %d iterations per run, child processes alternated:" % (what, a.train_iters))
    for form, v in runs.items():
        say("  %-45s ms per iteration: %s  (median %.3f, spread %.3f)" % (form, ", ".join("%.3f" % x for x in v), float(np.median(v)), max(v) - min(v)))
    return runs


if a.device_plan:
    from step_amd import DeviceRNG, DeviceTubeAugmentation
    NC = 60
    gt = np.zeros((N, 2, T, 4 + NC), np.float32)
    gt[..., :4] = tubes
    gt[..., 4 + 7] = 1
    d_gt, d_cnt = torch.from_numpy(gt).to(dev), torch.full((N,), 2, dtype=torch.int32, device=dev)
    host_aug = TubeAugmentation((Wo, Ho), do_flip=True, do_crop=True, do_photometric=True, do_erase=True, scale=2)
    dev_aug = DeviceTubeAugmentation((Wo, Ho), do_flip=True, do_crop=True, do_photometric=True, do_erase=True, scale=2, rng=DeviceRNG(dev, seed=11))
    g_out, c_out = torch.empty_like(d_gt), torch.empty_like(d_cnt)
    clips = list(frames.unbind(0))
    src, dims = None, None
    np.random.seed(11)

    def host_form():
        """what `--augment` does per batch ahead of the one launch: plan per clip, pack, the copy of the block (waited for here);
        its own host clock: ONE call split into the CPU part and the part that ends in the synchronise"""
        t0 = time.perf_counter()
        plans = [host_aug.plan((T, Hs, Ws), tubes[n])[0] for n in range(N)]
        t1 = time.perf_counter()
        _, block = host_aug.pack(frames, plans)
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, block.numel()

    dev_aug.apply(frames, d_gt, d_cnt, out=out, gt_out=g_out, gt_count_out=c_out)          # builds the static block, uploads the frame addresses
    block = dev_aug.last_block()
    src, dims = dev_aug._frames[1], dev_aug._frames[2]

    def plan_only():
        _capi.check(L.step_augment_plan(_lib.dptr(src), _lib.dptr(dims), _lib.dptr(d_gt), _lib.dptr(d_cnt), N, 2, T, NC, 15, 2, Wo, Ho, Hs * Ws,
                                        _lib.dptr(dev_aug.rng.state), _lib.dptr(block), _lib.dptr(g_out), _lib.dptr(c_out), _lib.stream_ptr(dev)),
                    "step_augment_plan")

    say("the augmentation's decisions for %d clips x %d frames of %dx%d, 2 tubes per clip, all four switches; %d rounds, alternated" % (N, T, Hs, Ws, a.rounds))
    timed(plan_only, 10)
    host_form()
    dev_ms, host_plan, host_copy, blk_bytes = [], [], [], []
    for _ in range(a.rounds):
        dev_ms.append(timed(plan_only, a.launches))
        hp = [host_form() for _ in range(5)]
        host_plan.append(float(np.median([h[0] for h in hp])))
        host_copy.append(float(np.median([h[1] for h in hp])))
        blk_bytes.append(int(np.median([h[2] for h in hp])))
    say("  device: step_augment_plan (planner + noise fill), median %.4f ms per batch (min %.4f .. max %.4f); static block %d bytes"
        % (float(np.median(dev_ms)), min(dev_ms), max(dev_ms), block.numel()))
    say("  host:   .plan x %d, median %.3f ms per batch (min %.3f .. max %.3f); pack + copy of the block, %.3f ms (min %.3f .. max %.3f; ~%d bytes)"
        % (N, float(np.median(host_plan)), min(host_plan), max(host_plan), float(np.median(host_copy)), min(host_copy), max(host_copy), int(np.median(blk_bytes))))
    res = {"device_plan_ms": dev_ms, "host_plan_ms": host_plan, "host_pack_copy_ms": host_copy}
    if a.plan_tubes:
        P, Tp = a.plan_tubes, 3
        xy = rs.uniform(0.0, 0.6, (N, P, 1, 2))
        props = np.tile(np.concatenate([xy, xy + rs.uniform(0.15, 0.35, (N, P, 1, 2))], 3), (1, 1, Tp, 1)).astype(np.float32)
        d_props, d_pcnt = torch.from_numpy(props).to(dev), torch.from_numpy(rs.randint(0, P + 1, N).astype(np.int32)).to(dev)
        d_fill = torch.from_numpy(np.tile(np.array([[0.1, 0.1, 0.8, 0.8]], np.float32), (min(P, 34), 1))).to(dev)
        t_out, tc_out = torch.empty_like(d_props), torch.empty_like(d_pcnt)

        def plan_tubes(n, with_tubes):
            t = (_lib.dptr(d_props), _lib.dptr(d_pcnt), P, Tp, _lib.dptr(d_fill), d_fill.shape[0], _lib.dptr(t_out), _lib.dptr(tc_out)) if with_tubes \
                else (None, None, 0, 0, None, 0, None, None)
            _capi.check(L.step_augment_plan_tubes(_lib.dptr(src), _lib.dptr(dims), _lib.dptr(d_gt), _lib.dptr(d_cnt), n, 2, T, NC, 15, 2, Wo, Ho, Hs * Ws,
                                                  _lib.dptr(dev_aug.rng.state), _lib.dptr(block), _lib.dptr(g_out), _lib.dptr(c_out), *t,
                                                  _lib.stream_ptr(dev)), "step_augment_plan_tubes")

        say("planner + noise fill with %d proposal slots per clip x %d frames (counts %s) against the same call without tubes; %d rounds x %d launches, alternated"
            % (P, Tp, d_pcnt.tolist(), a.rounds, a.launches))
        for n in (1, 8):
            forms = {"without tubes": lambda: plan_tubes(n, False), "with tubes": lambda: plan_tubes(n, True)}
            for fn in forms.values():
                timed(fn, 10)
            ms = {k: [] for k in forms}
            for _ in range(a.rounds):
                for k, fn in forms.items():
                    ms[k].append(timed(fn, a.launches))
            for k, v in ms.items():
                say("  %d clip(s), %-14s median %.4f ms per batch (min %.4f .. max %.4f)" % (n, k + ":", float(np.median(v)), min(v), max(v)))
            res["plan_tubes_%d" % n] = ms
    if a.train_runs:
        del frames, out
        torch.cuda.empty_cache()
        forms = ("--feed u8 --augment --select-device", "--feed u8 --augment-device --select-device")
        for clips_per_gpu in (1, 8):
            runs = train_children(forms, ["--global-batch", str(clips_per_gpu)], "%d clip(s) per GPU" % clips_per_gpu)
            h, d = runs[forms[0]], runs[forms[1]]
            say("  device-plan - host-plan = %+.3f ms per iteration; the host-plan form's own spread is %.3f ms"
                % (float(np.median(d) - np.median(h)), max(h) - min(h)))
            res["train_%d" % clips_per_gpu] = runs
    say(json.dumps(res))
    say.close()
    raise SystemExit(0)

forms = {
    "BaseTransform (resize only)": BaseTransform((Wo, Ho), scale=2),
    "geometry only (crop, mirror, erase)": TubeAugmentation((Wo, Ho), do_flip=True, do_crop=True, do_erase=True, scale=2),
    "all four switches": TubeAugmentation((Wo, Ho), do_flip=True, do_crop=True, do_photometric=True, do_erase=True, scale=2),
}
np.random.seed(11)
packed, plan_ms = {}, {}
for name, aug in forms.items():
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        plans = [aug.plan((T, Hs, Ws), tubes[n])[0] for n in range(N)]
    plan_ms[name] = (time.perf_counter() - t0) / (reps * N) * 1e3
    _, block = aug.pack(frames, plans)
    patch_bytes = sum(q.nbytes for p in plans for q in p.patches)
    src_bytes = sum(T * p.crop[2] * p.crop[3] * 3 for p in plans)              # the source pixels the crops cover, once
    packed[name] = (aug, block, plans, src_bytes + out.numel() * 2 + patch_bytes)
full = torch.from_numpy(rs.randint(0, 256, (N, T, Ho, Wo, 3)).astype(np.uint8)).to(dev)
calls = {name: (lambda v=v: v[0].launch(v[1], N, T, out)) for name, v in packed.items()}
calls["step_clip_from_u8 [8,36,400,400]"] = lambda: ops.clip_from_u8(full, scale=2, out=out)
need = {name: v[3] for name, v in packed.items()}
need["step_clip_from_u8 [8,36,400,400]"] = full.numel() + out.numel() * 2

# the box's streaming-copy rate, same process (bench.py's probe: 1 GiB read + 1 GiB written, 16 workgroups per CU, best of 5)
nbytes = 1 << 30
src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
cus = torch.cuda.get_device_properties(dev).multi_processor_count
stream = _lib.stream_ptr(dev)


def probe():
    _capi.check(L.step_hbm_stream_probe(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), nbytes, cus * 16, stream), "step_hbm_stream_probe")


probe()
hbm = max(2 * nbytes / (timed(probe, 3) * 1e-3) for _ in range(5))
say("step_clip_augment_u8 at %d clips x %d frames, %dx%d -> %dx%d, bf16 output; %d rounds x %d launches per form, alternated" % (N, T, Hs, Ws, Ho, Wo, a.rounds, a.launches))
say("step_hbm_stream_probe on this box, this process: %.2f TB/s (best of 5)" % (hbm / 1e12))
for fn in calls.values():                                                      # warm-up: every form, code objects loaded
    timed(fn, 10)
times = {k: [] for k in calls}
for _ in range(a.rounds):
    for k, fn in calls.items():
        times[k].append(timed(fn, a.launches))
say("%-40s %10s %20s %12s %10s %8s" % ("form", "median ms", "min .. max ms", "bytes needed", "TB/s", "of probe"))
res = {}
for k, v in times.items():
    med = float(np.median(v))
    rate = need[k] / (med * 1e-3)
    res[k] = dict(ms=med, min=min(v), max=max(v), bytes=need[k], share=rate / hbm)
    say("%-40s %10.4f %9.4f .. %-9.4f %12d %10.3f %7.1f%%" % (k, med, min(v), max(v), need[k], rate / 1e12, 100 * rate / hbm))
for name, (aug, block, plans, _) in packed.items():
    say("plan() host time, %-38s %.3f ms per clip (erase patches: %d bytes for the batch)" % (name + ":", plan_ms[name], sum(q.nbytes for p in plans for q in p.patches)))

from tests.augment_cases import np_apply  # noqa: E402
aug, _, plans, _ = packed["all four switches"]
t0 = time.perf_counter()
for n in range(a.np_clips):
    np_apply(frames_np[n], plans[n], aug.size, aug.scale, aug.mean, aug.stds)
np_ms = (time.perf_counter() - t0) / a.np_clips * 1e3
say("CPU time (this box's host, one thread of numpy): np_apply, all four switches, %.0f ms per clip -- the stand-in for what the reference's "
    "loader pays per clip; the device kernel takes %.3f ms per clip" % (np_ms, res["all four switches"]["ms"] / N))

if a.train_runs:
    del src, dst
    torch.cuda.empty_cache()
    runs = {"--feed u8": [], "--feed u8 --augment": []}
    for r in range(a.train_runs):
        for form in runs:
            cmd = [sys.executable, os.path.join(ROOT, "train_step_amd.py"), "--iters", str(a.train_iters), "--log-every", "0"] + form.split()
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                say("train_step_amd.py %s failed (%d): %s" % (form, p.returncode, (p.stdout + p.stderr)[-800:]))
                raise SystemExit(1)                                            # (nothing more is started after a failed child)
            s = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{") and "summary" in l][-1]
            runs[form].append(s["ms_per_iter"])
    say("train_step_amd.py, one clip per iteration, %d iterations per run, child processes alternated:" % a.train_iters)
    for form, v in runs.items():
        say("  %-22s ms per iteration: %s  (median %.3f, spread %.3f)" % (form, ", ".join("%.3f" % x for x in v), float(np.median(v)), max(v) - min(v)))
    plain, augd = runs["--feed u8"], runs["--feed u8 --augment"]
    diff = float(np.median(augd) - np.median(plain))
    say("  augmented - plain = %+.3f ms per iteration; the plain form's own spread is %.3f ms; the kernel's share at one clip: %.3f ms"
        % (diff, max(plain) - min(plain), res["all four switches"]["ms"] / N))
    res["train"] = runs
say(json.dumps({"hbm_probe_TBps": hbm / 1e12, "forms": res, "plan_ms_per_clip": plan_ms, "np_apply_ms_per_clip": np_ms}))
say.close()
