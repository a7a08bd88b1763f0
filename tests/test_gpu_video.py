"""The video demo's input side on the real gfx950 library: the cases of tests/video_cases.py (shared with the interpreter run of
tests/test_emul_video.py) plus what only exists on the device -- the count of clips()'s host synchronisations, and detect_video end to
end against the per-clip path through the same networks."""
import numpy as np
import pytest
import torch

from tests import video_cases as VC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", VC.KERNEL_CASES)
def test_gpu_video_kernel(name, bk):
    getattr(VC, name)(bk, "cuda")


@pytest.mark.parametrize("name", VC.MODULE_CASES)
def test_gpu_video_module(name, bk):
    getattr(VC, name)(bk, "cuda")


def test_clips_makes_no_host_synchronisation():
    """torch.cuda.set_sync_debug_mode("warn") reports every synchronising call: a warmed clips() over device-resident frames makes NONE
    (one non-blocking copy of the pinned slot table, one launch).  Two calls, so that both pinned tables are rewritten."""
    import warnings

    from step_amd import BaseTransform, VideoClips

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
    numf, Hs, Ws = 120, 64, 80
    vc = VideoClips(BaseTransform((400, 400), scale=2), 3, 3, 30, 12, numf, (Hs, Ws), "cuda", batch=2)
    fids = [50, 51]
    g = torch.Generator().manual_seed(3)
    for i in vc.needed(fids):
        vc.ring.push(i, torch.randint(0, 256, (Hs, Ws, 3), generator=g, dtype=torch.uint8).cuda())
    assert vc.ring.uploaded_frames == 0 and vc.needed(fids) == []
    out = torch.empty((2, 36, 3, 400, 400), dtype=torch.bfloat16, device="cuda")
    for _ in range(3):
        first = vc.clips(fids, out=out).clone()
    r = reports(lambda: [vc.clips(fids, out=out) for _ in range(2)])
    print("synchronising calls reported for clips():", len(r))
    assert r == []
    assert torch.equal(out, first)


def test_detect_video_equals_the_per_clip_path():
    """detect_video over a synthetic 6-frame video of 48x64 frames -> 400x400 (workloads.build_nets, batch 2, anchors "1"): its
    postprocess_merged dictionaries equal, bit for bit, those of the per-clip path through the same networks -- the frames of every clip
    stacked on the host, uploaded and put through BaseTransform.apply.  The clips are the same bits and inference is deterministic."""
    from step_amd import BaseTransform, VideoClips, detect_video, driver
    from step_amd.video import clip_frame_indices
    from step_amd.workloads import build_nets

    dev = torch.device("cuda:0")
    args, base, ctx, nets = build_nets(dev)
    nets = dict(nets, base_net=base, context_net=ctx)
    numf, Hs, Ws, batch = 6, 48, 64, 2
    rs = np.random.RandomState(31)
    video = rs.randint(0, 256, (numf, Hs, Ws, 3)).astype(np.uint8)
    aug = BaseTransform((400, 400), (0.05, -0.02, 0.03), (0.9, 1.1, 1.0), scale=2)
    chunks = args.NUM_CHUNKS[args.max_iter]
    vc = VideoClips(aug, args.T, chunks, 30, 12, numf, (Hs, Ws), dev, batch=batch, video_name="synthetic")
    seen = []

    def read_frame(i):
        seen.append(i)
        return video[i]

    got = list(detect_video(args, nets, vc, read_frame))
    assert [fid for fid, _ in got] == list(range(numf)) and seen == list(range(numf)) and vc.ring.uploaded_frames == numf
    want = []
    with torch.no_grad():
        for f0 in range(0, numf, batch):
            fids = list(range(f0, min(f0 + batch, numf)))
            stacked = np.stack([video[clip_frame_indices(f, numf, vc.frames, 30, 12)] for f in fids])
            images = aug.apply(torch.from_numpy(stacked).to(dev), [aug.plan(stacked.shape[1:4])[0] for _ in fids])
            cf = base(images)
            hist, _ = driver.inference(args, cf, ctx(cf), nets, args.max_iter, [vc.anchor_tubes.copy() for _ in fids])
            want += driver.postprocess_merged(args, hist, global_thresh=0.8, iterations=[len(hist) - 1])[0]
    assert len(want) == numf
    rows = 0
    for (fid, d), w in zip(got, want):
        assert set(d) == set(w) == {"boxes", "cluster", "labels", "scores", "tubes"}
        for k in w:
            assert d[k].dtype == w[k].dtype and torch.equal(d[k], w[k]), (fid, k)
        rows += int(d["scores"].numel())
    print("detections compared:", rows)
    assert rows > 0
