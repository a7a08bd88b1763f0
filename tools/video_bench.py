"""The video demo's input side at the demo shape -- 256x340 source frames -> 400x400, 36-frame clips at 30 -> 12 fps, bf16 -- ONE process, the
forms alternated round by round, the spread (min .. max of the rounds) reported beside the median:

  * kernels, every launch timed between device events after a warm-up: step_clip_gather_u8 over the ring (8 clips and 4 clips per launch,
    consecutive fids, so neighbouring clips share source frames) against step_clip_augment_u8 under BaseTransform plans on contiguous
    stacks of the same frames ("BaseTransform (resize only)" of profiles/clip_augment_timing.txt, re-measured here); for each, the bytes
    the algorithm needs (distinct source frames once + output once) over that time, as a share of what step_hbm_stream_probe moves on
    the same box in the same process;
  * loaders, wall clock per clip over a whole video of --numf frames held in host memory (decoding is not part of either), batch 4, with one
    device synchronisation per batch (where the demo hands the clips to the backbone):
      per-clip path   what exists without the ring: np.stack of the clip's 36 frames, upload, BaseTransform.apply
      ring path       VideoClips.batches: one upload per source frame, one table copy and one gather per batch
    and the host-to-device bytes per clip of each.

    python tools/video_bench.py [--out profiles/video_clips_timing.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from step_amd import BaseTransform, VideoClips, _capi, _lib
from step_amd.video import clip_frame_indices
from tools import abkit

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--launches", type=int, default=50, help="timed launches per form and round")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--numf", type=int, default=240, help="frames of the synthetic video the loaders run over")
ap.add_argument("--loader-rounds", type=int, default=3)
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/video_bench.py needs a ROCm device"
dev = torch.device("cuda:0")
L = _lib.lib()
say = abkit.tee(a.out)
timed = abkit.event_ms                                                         # ms per launch, no warm-up of its own: every form is warmed below

T, CHUNKS, SRC_FPS, DST_FPS, Hs, Ws, Ho, Wo, BATCH = 3, 3, 30, 12, 256, 340, 400, 400, 4
FRAMES = T * CHUNKS * 4
rs = np.random.RandomState(12)
video = rs.randint(0, 256, (a.numf, Hs, Ws, 3)).astype(np.uint8)
aug = BaseTransform((Wo, Ho), scale=2)


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------
calls, need = {}, {}
keep = []
for N in (8, 4):
    fids = list(range(a.numf // 2, a.numf // 2 + N))                          # mid-video: no clamping at either end
    idx = np.asarray([clip_frame_indices(f, a.numf, FRAMES, SRC_FPS, DST_FPS) for f in fids])
    vc = VideoClips(aug, T, CHUNKS, SRC_FPS, DST_FPS, a.numf, (Hs, Ws), dev, batch=N)
    for i in range(int(idx.min()), int(idx.max()) + 1):
        vc.ring.push(i, torch.from_numpy(video[i]).to(dev))
    out = torch.empty((N, FRAMES, 3, Ho, Wo), dtype=torch.bfloat16, device=dev)
    stacked = torch.from_numpy(video[idx]).to(dev)                            # [N,36,Hs,Ws,3]: the contiguous stacks of the same frames
    plans = [aug.plan((FRAMES, Hs, Ws))[0] for _ in range(N)]
    _, block = aug.pack(stacked, plans)
    ref = aug.launch(block, N, FRAMES, torch.empty_like(out)).clone()
    assert torch.equal(vc.clips(fids, out=out), ref), "the gather is not bit-equal to BaseTransform.apply on the stacked frames"
    table = torch.from_numpy(vc.ring.slots(idx).reshape(-1)).to(dev)
    m = (ctypes.c_float * 3)(*aug.mean)
    sd = (ctypes.c_float * 3)(*aug.stds)
    keep.append((vc, out, stacked, block, table, m, sd))

    def gather(vc=vc, out=out, table=table, m=m, sd=sd, N=N):
        _capi.check(L.step_clip_gather_u8(_lib.dptr(vc.ring.ring), vc.ring.slot_bytes, vc.ring.capacity, Hs, Ws, _lib.dptr(table), N, FRAMES, Ho, Wo,
                                          aug.scale, m, sd, 1, _capi.BF16, _lib.dptr(out), _lib.stream_ptr(dev)), "step_clip_gather_u8")

    distinct = len(np.unique(idx))
    calls["step_clip_gather_u8, %d clips (%d distinct frames)" % (N, distinct)] = gather
    need["step_clip_gather_u8, %d clips (%d distinct frames)" % (N, distinct)] = distinct * Hs * Ws * 3 + out.numel() * 2
    calls["BaseTransform (resize only), %d clips" % N] = lambda block=block, out=out, N=N: aug.launch(block, N, FRAMES, out)
    need["BaseTransform (resize only), %d clips" % N] = N * FRAMES * Hs * Ws * 3 + out.numel() * 2

nbytes = 1 << 30
src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
cus = torch.cuda.get_device_properties(dev).multi_processor_count
stream = _lib.stream_ptr(dev)


def probe():
    _capi.check(L.step_hbm_stream_probe(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), nbytes, cus * 16, stream), "step_hbm_stream_probe")


probe()
hbm = max(2 * nbytes / (timed(probe, 3) * 1e-3) for _ in range(5))
del src, dst
say("video clips at %dx%d -> %dx%d, %d-frame clips at %d -> %d fps, bf16 output; kernels: %d rounds x %d launches per form, alternated"
    % (Hs, Ws, Ho, Wo, FRAMES, SRC_FPS, DST_FPS, a.rounds, a.launches))
say("step_hbm_stream_probe on this box, this process: %.2f TB/s (best of 5)" % (hbm / 1e12))
for fn in calls.values():
    timed(fn, 10)
times = {k: [] for k in calls}
for _ in range(a.rounds):
    for k, fn in calls.items():
        times[k].append(timed(fn, a.launches))
say("%-50s %10s %20s %10s %12s %8s %8s" % ("form", "median ms", "min .. max ms", "us / clip", "bytes needed", "TB/s", "of probe"))
res = {}
for k, v in times.items():
    med = float(np.median(v))
    n_clips = 8 if " 8 clips" in k else 4
    rate = need[k] / (med * 1e-3)
    res[k] = dict(ms=med, min=min(v), max=max(v), us_per_clip=med * 1e3 / n_clips, bytes=need[k], share=rate / hbm)
    say("%-50s %10.4f %9.4f .. %-9.4f %10.1f %12d %8.3f %7.1f%%" % (k, med, min(v), max(v), med * 1e3 / n_clips, need[k], rate / 1e12, 100 * rate / hbm))
for N in (8, 4):
    g = [k for k in res if k.startswith("step_clip_gather_u8, %d" % N)][0]
    b = res["BaseTransform (resize only), %d clips" % N]
    say("%d clips: gather - BaseTransform = %+.4f ms (median); BaseTransform's own spread in this run is %.4f ms, the gather's %.4f ms"
        % (N, res[g]["ms"] - b["ms"], b["max"] - b["min"], res[g]["max"] - res[g]["min"]))
del keep, calls
torch.cuda.empty_cache()


# ---- loaders (their own host clock: one pass over the whole video with a synchronise per batch, returned with the bytes it moved) ------------
def per_clip_path():
    """np.stack of every clip's frames, upload, BaseTransform.apply -- batch by batch; returns (seconds, H2D bytes)."""
    moved = 0
    plans = [aug.plan((FRAMES, Hs, Ws))[0] for _ in range(BATCH)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f0 in range(0, a.numf, BATCH):
        fids = range(f0, min(f0 + BATCH, a.numf))
        stacked = np.stack([video[clip_frame_indices(f, a.numf, FRAMES, SRC_FPS, DST_FPS)] for f in fids])
        moved += stacked.nbytes
        aug.apply(torch.from_numpy(stacked).to(dev), plans[:len(fids)])
        torch.cuda.synchronize()
    return time.perf_counter() - t0, moved


def ring_path():
    vc = VideoClips(aug, T, CHUNKS, SRC_FPS, DST_FPS, a.numf, (Hs, Ws), dev, batch=BATCH)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for images, _, infos in vc.batches(lambda i: video[i]):
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert vc.ring.uploaded_frames == a.numf
    return dt, vc.ring.uploaded_bytes + a.numf * FRAMES * 4                    # frames once + the int32 slot tables


per_clip_path(), ring_path()                                                   # warm-up: allocator, pinned buffers
runs = {"per-clip path": [], "ring path": []}
moved = {}
for _ in range(a.loader_rounds):
    for k, fn in (("per-clip path", per_clip_path), ("ring path", ring_path)):
        dt, b = fn()
        runs[k].append(dt / a.numf * 1e3)
        moved[k] = b / a.numf
say("loaders over a %d-frame video in host memory, batch %d, %d rounds alternated (wall clock, one synchronisation per batch):" % (a.numf, BATCH, a.loader_rounds))
for k, v in runs.items():
    say("  %-14s %8.3f ms per clip (min %.3f .. max %.3f)   H2D %10.0f bytes per clip" % (k, float(np.median(v)), min(v), max(v), moved[k]))
say("  uploads per video: %d frames against %d (= %d x numf), by construction" % (a.numf, FRAMES * a.numf, FRAMES))
say(json.dumps({"hbm_probe_TBps": hbm / 1e12, "kernels": res, "loader_ms_per_clip": runs, "h2d_bytes_per_clip": moved}))
say.close()
