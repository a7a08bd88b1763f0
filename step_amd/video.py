"""step_amd/video.py -- the video demo's input side (data/customize.py:22-151 CustomizedDataset, demo.py:97-217) with the source frames
RESIDENT on the device.

The reference makes one clip per frame of the video: frame `fid` is the middle of a clip of T * chunks * 4 frames taken at a stride of
source_fps / target_fps, and `read_images` decodes, and BaseTransform resizes, every one of them again for every clip -- 36 * numf decodes,
resizes and uploads where numf would do, since neighbouring clips share almost all their source frames.  Here each decoded uint8 frame is
uploaded ONCE into a device ring (`FrameRing`), and a batch of clips is assembled by one launch of `step_clip_gather_u8`
(step_amd/csrc/pool.hip) that reads its frames through an index table: BaseTransform's resize and normalisation, bit for bit what
`BaseTransform.apply` gives on the stacked frames.  No CPU fallback.

    clips = VideoClips(BaseTransform((400, 400), MEANS, STDS, scale=2), T=3, chunks=3, source_fps=30, target_fps=12, numf=numf,
                       frame_size=(256, 340), device="cuda", batch=4, video_name="video1")
    for fid, result in detect_video(args, nets, clips, read_frame):       # read_frame(i) -> uint8 [Hs,Ws,3] BGR, called once per frame
        ...

The ring, the table copies and the gather are ordered by the CURRENT stream: pushes and gathers of one ring belong on one stream.
"""
import ctypes
import math

import numpy as np
import torch

from . import _capi, _lib
from .tube_math import anchor_tubes

__all__ = ["clip_frame_indices", "FrameRing", "VideoClips", "detect_video"]

TEM_REDUCE = 4                      # data/customize.py:20 (the I3D backbone's temporal reduction)
WIDTH, HEIGHT = 400, 400            # data/customize.py:19: the anchor tubes are scaled to this size, whatever the transform's
_DT = {torch.float32: _capi.F32, torch.bfloat16: _capi.BF16, torch.float16: _capi.F16}


def clip_frame_indices(fid, numf, frames, source_fps, target_fps):
    """The `frames` source-frame numbers of the clip centred on frame `fid` of a video of `numf` frames, in clip order
    (data/customize.py:83-103): a float stride, stepped down from fid for the left half and up for the right half, each position
    truncated by int() and clamped to 0 / numf - 1."""
    stride = source_fps / target_fps
    num_left = int(frames / 2)
    left, p = [], fid
    for _ in range(num_left):
        left.append(max(0, int(p)))
        p -= stride
    right, p = [], fid
    for _ in range(frames - num_left):
        p += stride
        right.append(min(numf - 1, int(p)))
    return left[::-1] + right


def _gather(ring, table, N, T, transform, out, rgb):
    """One launch of step_clip_gather_u8: table = int32 [N*T] on the ring's device, out [N,T,3,Ho,Wo]."""
    Wo, Ho = transform.size
    m = (ctypes.c_float * 3)(*transform.mean)
    sd = (ctypes.c_float * 3)(*transform.stds)
    _capi.check(_lib.lib().step_clip_gather_u8(_lib.dptr(ring.ring), ring.slot_bytes, ring.capacity, ring.Hs, ring.Ws, _lib.dptr(table), N, T, Ho, Wo,
                                               transform.scale, m, sd, 1 if rgb else 0, _DT[out.dtype], _lib.dptr(out),
                                               _lib.stream_ptr(out.device)), "step_clip_gather_u8")
    return out


def _out_for(ring, N, T, transform, dtype, out):
    Wo, Ho = transform.size
    if out is None:
        return torch.empty((N, T, 3, Ho, Wo), dtype=dtype, device=ring.device)
    if tuple(out.shape) != (N, T, 3, Ho, Wo) or not out.is_contiguous() or out.device != ring.device or out.dtype not in _DT:
        raise RuntimeError("step_amd: out= wants a contiguous fp32 / bf16 / fp16 [%d,%d,3,%d,%d] tensor on the ring's device" % (N, T, Ho, Wo))
    return out


class FrameRing:
    """`capacity` uint8 BGR frames [Hs,Ws,3] in device memory, at a pitch of slot_bytes (the frame size rounded up to 16).  Frame numbers are
    strictly increasing and frame k lives in slot k % capacity until frame k + capacity (or a later one of that slot) replaces it."""

    def __init__(self, capacity, Hs, Ws, device, staging=4):
        self.capacity, self.Hs, self.Ws = int(capacity), int(Hs), int(Ws)
        if self.capacity <= 0 or self.Hs <= 0 or self.Ws <= 0:
            raise ValueError("step_amd: FrameRing wants a positive capacity and frame size")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.frame_bytes = self.Hs * self.Ws * 3
        self.slot_bytes = (self.frame_bytes + 15) // 16 * 16
        self.ring = torch.zeros(self.capacity * self.slot_bytes, dtype=torch.uint8, device=self.device)
        if self.ring.data_ptr() % 16:
            raise RuntimeError("step_amd: the allocator returned a ring that is not 16-byte aligned")
        self.frame_of = np.full(self.capacity, -1, np.int64)          # frame number each slot holds (-1: none yet)
        self.last = -1                                                  # highest frame number pushed
        self.uploaded_frames = 0                                        # frames that came from host memory, and their bytes
        self.uploaded_bytes = 0
        self.pushed_frames = 0                                          # every push, device-resident sources included
        # host frames travel through a few pinned buffers: [buffer, event recorded after its last copy, or None]
        self._stage = [[None, None] for _ in range(max(int(staging), 1))] if self.device.type == "cuda" else []
        self._stage_at = 0

    def _slot_view(self, slot):
        return self.ring[slot * self.slot_bytes:slot * self.slot_bytes + self.frame_bytes].view(self.Hs, self.Ws, 3)

    def push(self, frame_no, frame):
        """frame: uint8 [Hs,Ws,3] (BGR, as decoded) -- a numpy array, a CPU tensor or a tensor on the ring's device."""
        frame_no = int(frame_no)
        if frame_no <= self.last:
            raise ValueError("step_amd: FrameRing.push(%d): frame numbers are strictly increasing, the last one was %d" % (frame_no, self.last))
        if isinstance(frame, np.ndarray):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        if not torch.is_tensor(frame) or frame.dtype != torch.uint8 or tuple(frame.shape) != (self.Hs, self.Ws, 3):
            raise RuntimeError("step_amd: FrameRing.push expects a uint8 [%d,%d,3] frame" % (self.Hs, self.Ws))
        slot = frame_no % self.capacity
        dst = self._slot_view(slot)
        if frame.device.type == "cpu":
            if self.device.type == "cuda":
                st = self._stage[self._stage_at % len(self._stage)]
                self._stage_at += 1
                if st[0] is None:
                    st[0] = torch.empty((self.Hs, self.Ws, 3), dtype=torch.uint8).pin_memory()
                    st[1] = torch.cuda.Event()
                elif not st[1].query():                               # the copy that last read this buffer: finished before it is rewritten
                    st[1].synchronize()
                st[0].copy_(frame)
                dst.copy_(st[0], non_blocking=True)
                st[1].record(torch.cuda.current_stream(self.device))
            else:
                dst.copy_(frame)
            self.uploaded_frames += 1
            self.uploaded_bytes += self.frame_bytes
        elif frame.device == self.device:
            dst.copy_(frame, non_blocking=True)
        else:
            raise RuntimeError("step_amd: FrameRing.push: the frame is on %s, the ring on %s" % (frame.device, self.device))
        self.frame_of[slot] = frame_no
        self.last = frame_no
        self.pushed_frames += 1

    def resident(self, frame_numbers):
        """bool per frame number: it is in the ring now."""
        f = np.asarray(frame_numbers, np.int64).reshape(-1)
        return (f >= 0) & (self.frame_of[f % self.capacity] == f)

    def slots(self, frame_numbers):
        """The int32 table step_clip_gather_u8 reads (host, same shape as frame_numbers).  Raises for a frame that was never pushed and for
        one that has been overwritten, naming it."""
        f = np.asarray(frame_numbers, np.int64)
        ok = self.resident(f).reshape(f.shape)
        if not ok.all():
            bad = int(f[~ok].reshape(-1)[0])
            held = int(self.frame_of[bad % self.capacity]) if bad >= 0 else -1
            if 0 <= bad < held:
                raise KeyError("step_amd: frame %d is no longer in the ring: frame %d has overwritten its slot (capacity %d)" % (bad, held, self.capacity))
            raise KeyError("step_amd: frame %d was never pushed into the ring (last frame pushed: %d)" % (bad, self.last))
        return (f % self.capacity).astype(np.int32)

    def gather(self, table, transform, dtype=torch.bfloat16, out=None, rgb=True):
        """One step_clip_gather_u8 launch over a slot table [N,T] given on the host (any integer array): transform = a BaseTransform (size,
        scale, mean, stds).  A slot outside [0, capacity) is refused here, before any launch."""
        t = np.asarray(table)
        if t.ndim != 2 or t.size == 0 or t.dtype.kind not in "iu":
            raise ValueError("step_amd: FrameRing.gather wants an integer slot table [N,T]")
        if int(t.min()) < 0 or int(t.max()) >= self.capacity:
            bad = int(t[(t < 0) | (t >= self.capacity)].reshape(-1)[0])
            raise ValueError("step_amd: slot %d is outside the ring's %d slots" % (bad, self.capacity))
        N, T = t.shape
        out = _out_for(self, N, T, transform, dtype, out)
        dev_table = torch.from_numpy(np.ascontiguousarray(t, np.int32).reshape(-1)).to(self.device)
        return _gather(self, dev_table, N, T, transform, out, rgb)


class VideoClips:
    """CustomizedDataset + DataLoader + detection_collate for ONE video whose frames a caller-supplied `read_frame(i)` decodes: every source
    frame is read and uploaded once, every batch of clips is one table copy and one launch.

    transform: a step_amd.BaseTransform (output size, scale, mean, stds); T, chunks, source_fps, target_fps, anchor_mode: CustomizedDataset's
    arguments (chunks = args.NUM_CHUNKS[args.max_iter]); numf: frames in the video; frame_size = (Hs, Ws) of the decoded frames."""

    def __init__(self, transform, T, chunks, source_fps, target_fps, numf, frame_size, device, batch=4, dtype=torch.bfloat16, anchor_mode="1",
                 video_name=""):
        self.transform, self.T, self.chunks = transform, int(T), int(chunks)
        self.source_fps, self.target_fps, self.numf = source_fps, target_fps, int(numf)
        self.frames = self.T * self.chunks * TEM_REDUCE
        self.batch, self.dtype, self.anchor_mode, self.video_name = int(batch), dtype, anchor_mode, video_name
        if self.numf <= 0 or self.batch <= 0 or self.frames <= 0 or dtype not in _DT:
            raise ValueError("step_amd: VideoClips wants numf, batch and T * chunks positive and an fp32 / bf16 / fp16 dtype")
        # the ring holds the span of `batch` consecutive clips: a clip reaches ceil(half * stride) frames to either side of its middle
        # frame (+1 each for the truncation of the float positions), and the batch moves the window by batch - 1 frames
        stride = source_fps / target_fps
        half = self.frames - int(self.frames / 2)
        span = 2 * (int(math.ceil(half * stride)) + 1)
        self.ring = FrameRing(min(span + self.batch, self.numf), frame_size[0], frame_size[1], device)
        self.device = self.ring.device
        self._cuda = self.device.type == "cuda"
        # the slot table of a batch: two pinned buffers used in turn, each guarded by an event recorded after its copy
        words = self.batch * self.frames
        self._tables = [[torch.empty(words, dtype=torch.int32).pin_memory() if self._cuda else torch.empty(words, dtype=torch.int32),
                         torch.cuda.Event() if self._cuda else None, False] for _ in range(2)]
        self._table_at = 0
        tubes = anchor_tubes(anchor_mode, self.T)                       # data/customize.py:129-146 (scale_tubes_abs: clamp to [0,1], then scale)
        tubes = np.minimum(np.maximum(tubes, 0.0), 1.0)
        for i in range(4):
            tubes[:, :, i] *= float(WIDTH) if i % 2 == 0 else float(HEIGHT)
        self.anchor_tubes = tubes

    def indices(self, fids):
        """[len(fids), frames] source-frame numbers (clip_frame_indices per clip)."""
        return np.asarray([clip_frame_indices(int(f), self.numf, self.frames, self.source_fps, self.target_fps) for f in fids], np.int64)

    def needed(self, fids):
        """The frame numbers the clips centred on `fids` read that are not in the ring, in increasing order."""
        idx = np.unique(self.indices(fids))
        return [int(v) for v in idx[~self.ring.resident(idx)]]

    def clips(self, fids, out=None):
        """The clips centred on `fids` (at most `batch`), [N,frames,3,Ho,Wo] in `dtype` (or `out`'s), RGB as data/customize.py:125 hands them
        over: one non-blocking copy of the slot table from pinned memory and one step_clip_gather_u8 launch.  Every frame they read
        must be in the ring (`needed`); a missing one raises and names the frame."""
        N = len(fids)
        if N == 0 or N > self.batch:
            raise ValueError("step_amd: VideoClips.clips takes 1 .. %d clips, got %d" % (self.batch, N))
        table = self.ring.slots(self.indices(fids)).reshape(-1)
        out = _out_for(self.ring, N, self.frames, self.transform, self.dtype, out)
        _lib.lib()
        tb = self._tables[self._table_at % 2]
        self._table_at += 1
        if self._cuda and tb[2] and not tb[1].query():                 # the copy that last read this buffer: finished before it is rewritten
            tb[1].synchronize()
        tb[0].numpy()[:table.size] = table
        if self._cuda:
            dev_table = tb[0][:table.size].to(self.device, non_blocking=True)
            tb[1].record(torch.cuda.current_stream(self.device))
            tb[2] = True
        else:
            dev_table = tb[0][:table.size].clone()
        return _gather(self.ring, dev_table, N, self.frames, self.transform, out, True)

    def batches(self, read_frame):
        """The loader loop: yields (images [N,frames,3,Ho,Wo], tubes, infos) per batch of consecutive frames, as the reference's DataLoader
        over CustomizedDataset with detection_collate does (shuffle off).  read_frame(i) -> uint8 [Hs,Ws,3] BGR is called exactly once per
        source frame, in increasing order."""
        for f0 in range(0, self.numf, self.batch):
            fids = list(range(f0, min(f0 + self.batch, self.numf)))
            for i in range(self.ring.last + 1, int(self.indices(fids).max()) + 1):      # (frames this batch skips are read by a later one)
                self.ring.push(i, read_frame(i))
            images = self.clips(fids)
            yield images, [self.anchor_tubes.copy() for _ in fids], [{"video_name": self.video_name, "fid": fid} for fid in fids]


def detect_video(args, nets, video_clips, read_frame, global_thresh=0.8, conf_thresh=None):
    """demo.py:109-217 as a generator over one video: per batch the base net, the context net (unless args.no_context), driver.inference over
    args.max_iter steps and driver.postprocess_merged of the last step; yields (fid, result) per clip, result = that clip's dictionary
    of postprocess_merged (driver.merged_csv writes the reference's text from it).  nets: 'base_net', 'context_net', 'roi_net', 'det_net0' ...;
    conf_thresh None = args.conf_thresh (demo.py:54 uses 0.4).  Files, drawing and a second batch in flight are the caller's."""
    from . import driver

    with torch.no_grad():
        for images, tubes, infos in video_clips.batches(read_frame):
            conv_feat = nets["base_net"](images)
            context_feat = None if args.no_context else nets["context_net"](conv_feat)
            history, _ = driver.inference(args, conv_feat, context_feat, nets, args.max_iter, tubes)
            dets = driver.postprocess_merged(args, history, conf_thresh=conf_thresh, global_thresh=global_thresh, iterations=[len(history) - 1])[0]
            for info, det in zip(infos, dets):
                yield info["fid"], det
