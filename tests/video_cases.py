"""Video demo input on the device (step_amd/video.py, step_clip_gather_u8): the cases shared by the interpreter run
(tests/test_emul_video.py) and the run on the real gfx950 library (tests/test_gpu_video.py).

  * kernel cases: the C entry point driven directly over a hand-built ring.  The expected output is always the EXISTING
    `BaseTransform.apply` (step_clip_augment_u8 under the identity plan) on `torch.stack` of the indexed frames, compared on raw bits --
    the gather's contract is bit identity with that call, so no tolerance exists to choose.  Every launch writes into a buffer that sits
    between two sentinel pads, and the pads are checked after it.
  * module cases: `clip_frame_indices` against the lists the reference's own `CustomizedDataset.read_images` produced
    (tests/golden/video_index_golden.json, tools/make_video_golden.py), `FrameRing` / `VideoClips` against the per-clip path the
    reference's loader takes (stack the clip's frames on the host, transform them), and the bookkeeping: one upload per source frame.
Cases take (bk, device): the ctypes backend of tests/backends.py and the torch device the module-level calls run on ("cpu" inside
tests.emul.patch.emulated_kernels, "cuda" on the GPU)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from step_amd import BaseTransform, _capi
from step_amd.video import FrameRing, VideoClips, clip_frame_indices
from tests.augment_cases import _addr, _bits

F32, BF16, F16 = _capi.F32, _capi.BF16, _capi.F16
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
MEAN, STDS = (0.1, -0.2, 0.3), (0.9, 0.5, 2.0)
PAD = 64                                                    # sentinel elements on either side of the output (keeps its 16-byte alignment)
E_DTYPE, E_SHAPE, E_NULL = -1, -2, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_index_golden.json")


def fixture():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- driving the C ABI ---------------------------------------------------------------------------------------------------------------
def make_ring(frames, n_slots, slot_bytes, poison=0xA5):
    """frames: {slot: uint8 [Hs,Ws,3]} -> the ring as a flat uint8 array; every byte no frame owns (other slots, the gap up to the pitch)
    holds `poison`."""
    ring = np.full(n_slots * slot_bytes, poison, np.uint8)
    for s, fr in frames.items():
        ring[s * slot_bytes:s * slot_bytes + fr.size] = fr.reshape(-1)
    return ring


def run_gather(bk, ring, slot_bytes, n_slots, Hs, Ws, table, size, scale, mean=MEAN, stds=STDS, rgb=False, dtype=F32, expect=0):
    """One step_clip_gather_u8 call into a buffer between sentinel pads; returns the [N,T,3,Ho,Wo] output (fp32, or the 16-bit patterns
    as uint16) after checking the status and the pads.  expect != 0: the status is that error and NOTHING was written."""
    Wo, Ho = size
    table = np.ascontiguousarray(table, np.int32)
    N, T = table.shape
    n = N * T * 3 * Ho * Wo
    if dtype == F32:
        host = np.full(n + 2 * PAD, -77.25, np.float32)
    else:
        host = np.full(n + 2 * PAD, 0xABCD, np.uint16)
    before = host.copy()
    d_ring, d_table, d_out = bk.dev(ring), bk.dev(table.reshape(-1)), bk.dev(host)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_float * 3)(*[float(v) for v in stds])
    out_ptr = ctypes.c_void_p(_addr(d_out.ptr) + PAD * host.itemsize)
    rc = bk.lib.step_clip_gather_u8(d_ring.ptr, slot_bytes, n_slots, Hs, Ws, d_table.ptr, N, T, Ho, Wo, scale, m, sd, int(rgb), dtype, out_ptr, bk.stream)
    assert rc == expect, (rc, expect)
    got = d_out.get()
    if expect != 0:
        assert np.array_equal(got.view(np.uint8), before.view(np.uint8)), "an error return wrote to the output"
        return None
    assert np.array_equal(got[:PAD].view(np.uint8), before[:PAD].view(np.uint8)), "the pad in front of the output was written"
    assert np.array_equal(got[PAD + n:].view(np.uint8), before[PAD + n:].view(np.uint8)), "the pad behind the output was written"
    return got[PAD:PAD + n].reshape(N, T, 3, Ho, Wo).copy()


def want_bits(device, stacked, size, scale, mean=MEAN, stds=STDS, rgb=False, dtype=F32):
    """The existing path: BaseTransform.apply on the contiguous stack [N,T,Hs,Ws,3] of the frames the table names."""
    aug = BaseTransform(size, mean, stds, scale=scale)
    N, T, Hs, Ws, _ = stacked.shape
    plans = [aug.plan((T, Hs, Ws))[0] for _ in range(N)]
    out = aug.apply(torch.from_numpy(np.ascontiguousarray(stacked)).to(device), plans, dtype=TORCH_DT[dtype], rgb=rgb)
    return _bits(out)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def _frames(seed, n, Hs, Ws):
    return np.random.RandomState(seed).randint(0, 256, (n, Hs, Ws, 3)).astype(np.uint8)


def case_indexed_gather_with_resize(bk, device):
    """7 slots of 9x11 frames (33-byte rows) at a pitch of 304 bytes, N = 2, T = 5 -> 8x12 (H shrinks, W grows); tables with repeats, a
    non-monotone order and the last slot; every dtype, rgb 0 / 1, scale 0 / 1 / 2, non-trivial mean and stds."""
    Hs, Ws, n_slots, slot_bytes = 9, 11, 7, 304
    fr = _frames(21, n_slots, Hs, Ws)
    ring = make_ring({s: fr[s] for s in range(n_slots)}, n_slots, slot_bytes)
    table = np.array([[0, 0, 1, 3, 6], [6, 2, 2, 5, 4]], np.int32)
    for dtype in (F32, BF16, F16):
        for rgb in (False, True):
            for scale in (0, 1, 2):
                got = run_gather(bk, ring, slot_bytes, n_slots, Hs, Ws, table, (12, 8), scale, rgb=rgb, dtype=dtype)
                assert same_bits(got, want_bits(device, fr[table], (12, 8), scale, rgb=rgb, dtype=dtype)), (dtype, rgb, scale)


def case_more_than_one_workgroup(bk, device):
    """N = 3, T = 4 -> 16x24: 576 threads, three workgroups with a partial last one; slots in reverse."""
    Hs, Ws, n_slots, slot_bytes = 9, 11, 5, 304
    fr = _frames(22, n_slots, Hs, Ws)
    ring = make_ring({s: fr[s] for s in range(n_slots)}, n_slots, slot_bytes)
    table = np.array([[4, 3, 2, 1], [0, 4, 0, 4], [1, 1, 3, 2]], np.int32)
    for dtype in (F32, BF16):
        got = run_gather(bk, ring, slot_bytes, n_slots, Hs, Ws, table, (24, 16), 2, rgb=True, dtype=dtype)
        assert same_bits(got, want_bits(device, fr[table], (24, 16), 2, rgb=True, dtype=dtype)), dtype


def case_equal_sizes_copy(bk, device):
    """Source size == output size (no resize): 8x16 (whole 16-byte runs), 6x10 (a partial last run) and Wo = 13 with N = T = 1."""
    for (H, W, table) in ((8, 16, [[2, 0], [1, 1]]), (6, 10, [[1, 2], [0, 2]]), (5, 13, [[1]])):
        n_slots = 3
        slot_bytes = (H * W * 3 + 15) // 16 * 16 + 16
        fr = _frames(23 + W, n_slots, H, W)
        ring = make_ring({s: fr[s] for s in range(n_slots)}, n_slots, slot_bytes)
        table = np.array(table, np.int32)
        for dtype in (F32, BF16, F16):
            for scale in (0, 2):
                got = run_gather(bk, ring, slot_bytes, n_slots, H, W, table, (W, H), scale, rgb=True, dtype=dtype)
                assert same_bits(got, want_bits(device, fr[table], (W, H), scale, rgb=True, dtype=dtype)), (H, W, dtype, scale)


def case_no_stray_reads_or_writes(bk, device):
    """The slots the table does not name, and the bytes between a frame's end and the pitch, hold one poison value in the first run and
    another in the second: the outputs are equal (and right).  run_gather checks the sentinel pads around the output every time."""
    Hs, Ws, n_slots, slot_bytes = 9, 11, 7, 304
    fr = _frames(24, n_slots, Hs, Ws)
    table = np.array([[4, 1, 4]], np.int32)
    outs = []
    for poison in (0x00, 0xFF):
        ring = make_ring({1: fr[1], 4: fr[4]}, n_slots, slot_bytes, poison)
        outs.append([run_gather(bk, ring, slot_bytes, n_slots, Hs, Ws, table, size, 2, dtype=dt) for size in ((12, 8), (11, 9)) for dt in (F32, BF16)])
    for a, b in zip(*outs):
        assert same_bits(a, b)
    assert same_bits(outs[0][0], want_bits(device, fr[table], (12, 8), 2)) and same_bits(outs[0][2], want_bits(device, fr[table], (11, 9), 2))


def case_error_codes(bk, device):
    """Every refusal of include/step_amd.h, each with an untouched output (run_gather compares the whole buffer)."""
    Hs, Ws, n_slots, slot_bytes = 9, 11, 2, 304
    fr = _frames(25, n_slots, Hs, Ws)
    ring = make_ring({0: fr[0], 1: fr[1]}, n_slots, slot_bytes)
    table = np.array([[1, 0]], np.int32)

    def call(expect, ring=ring, slot_bytes=slot_bytes, n_slots=n_slots, Hs=Hs, Ws=Ws, size=(12, 8), scale=2, dtype=F32):
        return run_gather(bk, ring, slot_bytes, n_slots, Hs, Ws, table, size, scale, dtype=dtype, expect=expect)

    assert call(0) is not None
    for kw in (dict(n_slots=0), dict(Hs=0), dict(Ws=-1), dict(size=(0, 8)), dict(size=(12, 0)), dict(scale=3), dict(scale=-1),
               dict(slot_bytes=288), dict(slot_bytes=296), dict(slot_bytes=300), dict(slot_bytes=312)):    # 288, 296 < 297 = 9*11*3; 300, 312: no multiple of 16
        call(E_SHAPE, **kw)
    # the dtype code is step_clip_augment_u8's
    src = bk.dev(fr[0])
    from tests.augment_cases import AugPlan, pack_block
    block = bk.dev(pack_block([AugPlan(Hs, Ws)], [_addr(src.ptr)]))
    o = bk.dev(np.zeros((1, 1, 3, 8, 12), np.float32))
    assert bk.lib.step_clip_augment_u8(block.ptr, 1, 1, 8, 12, 2, None, None, 0, 7, o.ptr, bk.stream) == E_DTYPE
    call(E_DTYPE, dtype=7)
    # sizes and NULL pointers through the raw call
    d_ring, d_table = bk.dev(ring), bk.dev(table.reshape(-1))
    host = np.full(2 * 3 * 8 * 12, 5.0, np.float32)
    d_out = bk.dev(host)
    raw = bk.lib.step_clip_gather_u8
    assert raw(d_ring.ptr, slot_bytes, n_slots, Hs, Ws, d_table.ptr, -1, 2, 8, 12, 2, None, None, 0, F32, d_out.ptr, bk.stream) == E_SHAPE
    assert raw(d_ring.ptr, slot_bytes, n_slots, Hs, Ws, d_table.ptr, 1, 0, 8, 12, 2, None, None, 0, F32, d_out.ptr, bk.stream) == E_SHAPE
    assert raw(None, slot_bytes, n_slots, Hs, Ws, d_table.ptr, 1, 2, 8, 12, 2, None, None, 0, F32, d_out.ptr, bk.stream) == E_NULL
    assert raw(d_ring.ptr, slot_bytes, n_slots, Hs, Ws, None, 1, 2, 8, 12, 2, None, None, 0, F32, d_out.ptr, bk.stream) == E_NULL
    assert raw(d_ring.ptr, slot_bytes, n_slots, Hs, Ws, d_table.ptr, 1, 2, 8, 12, 2, None, None, 0, F32, None, bk.stream) == E_NULL
    assert raw(None, slot_bytes, n_slots, Hs, Ws, None, 0, 2, 8, 12, 2, None, None, 0, F32, None, bk.stream) == 0      # an empty batch is no error
    assert np.array_equal(d_out.get(), host)


def case_out_of_range_slot(bk, device):
    """A slot outside [0, n_slots): the Python layer refuses the table before any launch.  The direct C call clamps -- checked on the host
    interpreter ONLY (a table the product never sends is not put in front of the real device): same output as the clamped table."""
    Hs, Ws, n_slots = 9, 11, 4
    fr = _frames(26, n_slots, Hs, Ws)
    ring = FrameRing(n_slots, Hs, Ws, device)
    for k in range(n_slots):
        ring.push(k, fr[k])
    aug = BaseTransform((12, 8), MEAN, STDS, scale=2)
    good = ring.gather(np.array([[3, 0, 2]]), aug, dtype=torch.float32, rgb=False)
    assert same_bits(_bits(good), want_bits(device, fr[np.array([[3, 0, 2]])], (12, 8), 2))
    for bad in ([[3, 4, 2]], [[-1, 0, 2]], [[3, 0, 1 << 20]]):
        with pytest.raises(ValueError, match="slot"):
            ring.gather(np.array(bad), aug, dtype=torch.float32)
    with pytest.raises(ValueError):
        ring.gather(np.array([[0.5, 1.0]]), aug)
    if bk.name == "emul":
        flat = make_ring({s: fr[s] for s in range(n_slots)}, n_slots, ring.slot_bytes)
        wild = run_gather(bk, flat, ring.slot_bytes, n_slots, Hs, Ws, np.array([[-3, 9, 2, 1 << 30, -(1 << 31)]]), (12, 8), 2)
        clamped = run_gather(bk, flat, ring.slot_bytes, n_slots, Hs, Ws, np.array([[0, 3, 2, 3, 0]]), (12, 8), 2)
        assert same_bits(wild, clamped)


KERNEL_CASES = ["case_indexed_gather_with_resize", "case_more_than_one_workgroup", "case_equal_sizes_copy", "case_no_stray_reads_or_writes",
                "case_error_codes", "case_out_of_range_slot"]


# ---- the module ------------------------------------------------------------------------------------------------------------------------
def check_index_parity():
    """clip_frame_indices == every list the reference's read_images produced (4 rate pairs x 36 / 12 frames x 6 (fid, numf) points)."""
    g = fixture()
    assert len(g["cases"]) == 48
    for c in g["cases"]:
        got = clip_frame_indices(c["fid"], c["numf"], c["frames"], c["source_fps"], c["target_fps"])
        assert got == c["indices"], (c, got)


def module_ring_feeds_every_clip_once(bk, device):
    """numf = 40 frames of 10x14 -> 8x8, 12-frame clips (T = 1, chunks = 3) at 30 -> 12 fps, batch 2, over all fids: every batch is bit-equal
    to the per-clip path (stack the clip's frames on the host, BaseTransform.apply); the ring took numf uploads where that path moves
    12 * numf frames; read_frame saw each index once, in order; tubes and infos are the loader's."""
    numf, Hs, Ws, T, chunks, batch = 40, 10, 14, 1, 3, 2
    video = _frames(27, numf, Hs, Ws)
    aug = BaseTransform((8, 8), MEAN, STDS, scale=2)
    vc = VideoClips(aug, T, chunks, 30, 12, numf, (Hs, Ws), device, batch=batch, video_name="v")
    assert vc.frames == 12 and vc.ring.capacity < numf                       # (frames ARE evicted in this run)
    seen = []

    def read_frame(i):
        seen.append(i)
        return video[i] if i % 2 else torch.from_numpy(video[i])            # numpy arrays and CPU tensors alike

    tubes_want = np.asarray(fixture()["anchor_tubes"]["1"]["values"]).reshape(fixture()["anchor_tubes"]["1"]["shape"])[:, :T]
    fid, moved = 0, 0
    for images, tubes, infos in vc.batches(read_frame):
        n = len(infos)
        assert tuple(images.shape) == (n, 12, 3, 8, 8) and images.dtype == torch.bfloat16 and images.device.type == torch.device(device).type
        for k in range(n):
            idx = clip_frame_indices(fid, numf, 12, 30, 12)
            per_clip = aug.apply(torch.from_numpy(video[idx][None]).to(device), [aug.plan((12, Hs, Ws))[0]])      # bf16, rgb: the defaults
            moved += len(idx)
            assert same_bits(_bits(images[k:k + 1]), _bits(per_clip)), fid
            assert infos[k] == {"video_name": "v", "fid": fid}
            assert tubes[k].shape == tubes_want.shape and np.array_equal(np.asarray(tubes[k], np.float64), tubes_want)
            fid += 1
    assert fid == numf and seen == list(range(numf))
    assert vc.ring.uploaded_frames == numf and vc.ring.uploaded_bytes == numf * Hs * Ws * 3 and moved == 12 * numf
    # frame 0 has been overwritten by now; a fresh ring holds nothing yet.  Both refusals name the frame
    with pytest.raises(KeyError, match="frame 0 is no longer in the ring"):
        vc.clips([0])
    with pytest.raises(KeyError, match="frame 0 "):
        vc.ring.slots([39, 0])
    fresh = VideoClips(aug, T, chunks, 30, 12, numf, (Hs, Ws), device, batch=batch)
    assert fresh.needed([0]) == sorted(set(clip_frame_indices(0, numf, 12, 30, 12)))
    with pytest.raises(KeyError, match="frame 0 was never pushed"):
        fresh.clips([0])
    fresh.ring.push(0, video[0])
    with pytest.raises(KeyError, match="frame 2 was never pushed"):
        fresh.clips([0])
    with pytest.raises(ValueError, match="strictly increasing"):
        fresh.ring.push(0, video[0])


def module_device_frames_and_out(bk, device):
    """Frames pushed as tensors on the ring's device (no upload counted), `out=` filled in place with its own dtype, clips of a batch in
    any order of fids."""
    numf, Hs, Ws = 9, 6, 10
    video = _frames(28, numf, Hs, Ws)
    aug = BaseTransform((10, 6), MEAN, STDS, scale=1)                         # equal sizes: the copy path through the module
    vc = VideoClips(aug, 3, 1, 12, 12, numf, (Hs, Ws), device, batch=3, dtype=torch.float32)
    assert vc.ring.capacity == numf
    for i in range(numf):
        vc.ring.push(i, torch.from_numpy(video[i]).to(device))
    assert vc.ring.uploaded_frames == (numf if torch.device(device).type == "cpu" else 0) and vc.ring.pushed_frames == numf and vc.needed(range(numf)) == []
    out = torch.full((3, 12, 3, 6, 10), 7.0, dtype=torch.float16, device=device)
    fids = [8, 0, 4]
    assert vc.clips(fids, out=out) is out
    idx = np.asarray([clip_frame_indices(f, numf, 12, 12, 12) for f in fids])
    assert same_bits(_bits(out), want_bits(device, video[idx], (10, 6), 1, rgb=True, dtype=F16))
    assert same_bits(_bits(vc.clips(fids[:2])), want_bits(device, video[idx[:2]], (10, 6), 1, rgb=True, dtype=F32))
    with pytest.raises(RuntimeError):
        vc.clips(fids, out=torch.zeros((3, 12, 3, 6, 9), device=device))
    with pytest.raises(ValueError):
        vc.clips([0, 1, 2, 3])
    with pytest.raises(RuntimeError):
        vc.ring.push(numf, torch.zeros((Hs, Ws + 1, 3), dtype=torch.uint8))


MODULE_CASES = ["module_ring_feeds_every_clip_once", "module_device_frames_and_out"]
