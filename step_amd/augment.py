"""step_amd/augment.py -- the training loader's transform (data/augmentations.py:540-586 TubeAugmentation, :601-615 BaseTransform)
split in two: a HOST PLAN and one DEVICE launch.

Every random decision of that pipeline -- photometric parameters, crop rectangle, mirror, erase rectangles -- depends on the frame
shape and the tubes only, never on a pixel.  `.plan()` therefore draws them from numpy's global RNG in exactly the reference's order
(the same seed gives the same decisions, the same transformed tubes, and leaves the stream where the reference leaves it), which a
dataset worker can do without touching a frame; `.apply()` packs the plans of a batch into one pinned block, copies it with one
non-blocking transfer and applies all of them to the uint8 source frames with ONE launch of `step_clip_augment_u8`
(step_amd/csrc/pool.hip), writing the `[N,T,3,Ho,Wo]` clip `BaseNet.forward` takes.  No host synchronisation, no CPU fallback.

    aug = TubeAugmentation((400, 400), MEANS, STDS, do_flip=True, do_crop=True, do_photometric=True, do_erase=True, scale=2)
    plan, tubes, proposals = aug.plan(frames_u8.shape[:3], gt_tubes, proposals)      # in the dataset worker (host, cheap)
    clip = aug.apply(list_of_device_u8_clips, list_of_plans)                         # in the training loop (device)
"""
import ctypes

import numpy as np
import torch

from . import _capi, _lib

__all__ = ["AugPlan", "TubeAugmentation", "BaseTransform", "DeviceTubeAugmentation"]

F_MIRROR, F_PHOTOMETRIC, F_BRIGHTNESS, F_CONTRAST, F_CONTRAST_FIRST, F_SATURATION, F_HUE = 1, 2, 4, 8, 16, 32, 64    # include/step_amd.h
_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
_CROP_MIN_IOU = (None, 0.1, 0.3, 0.5, 0.7, 0.9, float("-inf"))      # RandomSampleCrop's modes; None = keep the whole frame
_NOISE_RANGE = {0: (0, 255), 1: (0, 1), 2: (-1, 1)}
_CLIP_WORDS, _RECT_WORDS = 16, 6


class AugPlan:
    """What one clip's transform does to its pixels.  crop = (x, y, w, h) in the source frame; the photometric parameters are float32
    (the reference's in-place numpy operations round the Python-float draw to the image's dtype) or None where the coin said no;
    rects = [(x1, y1, x2, y2)] in the cropped, mirrored frame with patches[k] float32 [y2-y1, x2-x1, 3]."""
    __slots__ = ("Hs", "Ws", "crop", "mirror", "photometric", "brightness", "contrast", "contrast_first", "saturation", "hue", "perm",
                 "rects", "patches")

    def __init__(self, Hs, Ws):
        self.Hs, self.Ws = int(Hs), int(Ws)
        self.crop = (0, 0, self.Ws, self.Hs)
        self.mirror = False
        self.photometric = False
        self.brightness = self.contrast = self.saturation = self.hue = None
        self.contrast_first = False
        self.perm = (0, 1, 2)
        self.rects, self.patches = [], []

    def flags(self):
        f = (F_MIRROR if self.mirror else 0) | (F_PHOTOMETRIC if self.photometric else 0)
        f |= (F_BRIGHTNESS if self.brightness is not None else 0) | (F_CONTRAST if self.contrast is not None else 0)
        f |= (F_CONTRAST_FIRST if self.contrast_first else 0) | (F_SATURATION if self.saturation is not None else 0)
        return f | (F_HUE if self.hue is not None else 0)

    def check(self):
        x, y, w, h = self.crop
        if not (0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= self.Ws and y + h <= self.Hs):
            raise ValueError("step_amd: crop %r outside the %dx%d source frame" % (self.crop, self.Hs, self.Ws))
        for (x1, y1, x2, y2), p in zip(self.rects, self.patches):
            if not (0 <= x1 <= x2 <= w and 0 <= y1 <= y2 <= h):
                raise ValueError("step_amd: erase rectangle %r outside the %dx%d crop" % ((x1, y1, x2, y2), h, w))
            if p.dtype != np.float32 or p.shape != (y2 - y1, x2 - x1, 3):
                raise ValueError("step_amd: erase patch %r %s does not fit its rectangle" % (p.shape, p.dtype))


def _mid_boxes(tubes):
    return tubes[:, int(tubes.shape[1] / 2), :4]


def _scale_xy(a, width, height, divide):
    for k, v in ((0, width), (2, width), (1, height), (3, height)):
        if divide:
            a[:, :, k] /= v
        else:
            a[:, :, k] *= v


def _shift_into(a, rect):
    """Clamp the boxes of a [n, T, >=4] array to the integer rectangle and move them to its origin (in place, in the array's dtype)."""
    a[:, :, :2] = np.maximum(a[:, :, :2], rect[:2])
    a[:, :, :2] -= rect[:2]
    a[:, :, 2:4] = np.minimum(a[:, :, 2:4], rect[2:])
    a[:, :, 2:4] -= rect[:2]


def _valid_tubes(tubes, width, height):
    """utils/tube_utils.py:59-92 on a numpy array: clamp to the window, replace boxes thinner than 2 by the whole window."""
    n, T, _ = tubes.shape
    b = tubes.reshape(-1, 4)
    b[:, 0] = np.maximum(0, b[:, 0])
    b[:, 1] = np.maximum(0, b[:, 1])
    b[:, 2] = np.minimum(width, b[:, 2])
    b[:, 3] = np.minimum(height, b[:, 3])
    bad = ~((b[:, 0] < b[:, 2] - 2) & (b[:, 1] < b[:, 3] - 2))
    b[bad, :2] = 0
    b[bad, 2] = width
    b[bad, 3] = height
    return b.reshape(n, T, 4)


class _Transform:
    def __init__(self, size, mean, stds, scale):
        self.size = (int(size[0]), int(size[1]))           # (width, height), as the reference's Resize takes it
        self.mean = tuple(float(np.float32(v)) for v in mean)
        self.stds = tuple(float(np.float32(v)) for v in stds)
        self.scale = int(scale)
        if self.scale not in (0, 1, 2):
            raise ValueError("step_amd: scale must be 0 ([0,255]), 1 ([0,1]) or 2 ([-1,1])")
        self._ring = []                                     # [(pinned block, event of its last copy)]

    # ---- device side ------------------------------------------------------------------------------------------------------------
    def _pinned(self, nbytes, cuda):
        if not cuda:
            return torch.empty(nbytes, dtype=torch.uint8), None
        for k, (buf, ev) in enumerate(self._ring):
            if buf.numel() >= nbytes and ev.query():         # (its last copy has finished: free to overwrite; never waited for)
                return buf, k
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8).pin_memory()
        self._ring.append((buf, torch.cuda.Event()))
        if len(self._ring) > 8:
            self._ring.pop(0)
        return buf, len(self._ring) - 1

    def pack(self, frames, plans):
        """The plan block of include/step_amd.h for a batch -- step_aug_clip[N] | step_aug_rect[...] | patches, in 4-byte words --
        written into one pinned buffer and copied with one non-blocking transfer.  Returns (clips, device block)."""
        clips = list(frames.unbind(0)) if torch.is_tensor(frames) else list(frames)
        N = len(clips)
        if N == 0 or len(plans) != N:
            raise RuntimeError("step_amd: apply() wants one plan per clip (%d clips, %d plans)" % (N, len(plans)))
        T, dev = clips[0].shape[0], clips[0].device
        for c, p in zip(clips, plans):
            if c.dtype != torch.uint8 or c.dim() != 4 or c.shape[-1] != 3 or not c.is_contiguous() or c.device != dev or c.shape[0] != T:
                raise RuntimeError("step_amd: apply() expects contiguous uint8 clips [T,H,W,3] of one length on one device")
            if (c.shape[1], c.shape[2]) != (p.Hs, p.Ws):
                raise RuntimeError("step_amd: plan drawn for %dx%d frames, clip has %dx%d" % (p.Hs, p.Ws, c.shape[1], c.shape[2]))
            p.check()                                        # (the kernel trusts the block: nothing outside a frame, a crop or the block)
        n_rects = sum(len(p.rects) for p in plans)
        words = _CLIP_WORDS * N + _RECT_WORDS * n_rects + sum(p_.size for p in plans for p_ in p.patches)
        host, slot = self._pinned(4 * words, dev.type == "cuda")
        blk = host.numpy()[:4 * words]
        w32, f32 = blk.view(np.int32), blk.view(np.float32)
        rect_at, patch_at = _CLIP_WORDS * N, _CLIP_WORDS * N + _RECT_WORDS * n_rects
        for n, (c, p) in enumerate(zip(clips, plans)):
            o = _CLIP_WORDS * n
            blk[4 * o:4 * o + 8].view(np.uint64)[0] = c.data_ptr()
            w32[o + 2:o + 10] = (p.Hs, p.Ws) + tuple(p.crop) + (p.flags(), p.perm[0] | p.perm[1] << 2 | p.perm[2] << 4)
            f32[o + 10:o + 14] = [0.0 if v is None else v for v in (p.brightness, p.contrast, p.saturation, p.hue)]
            w32[o + 14:o + 16] = (len(p.rects), rect_at)
            for r, patch in zip(p.rects, p.patches):
                w32[rect_at:rect_at + _RECT_WORDS] = tuple(r) + (patch_at, 0)
                f32[patch_at:patch_at + patch.size] = patch.reshape(-1)
                rect_at += _RECT_WORDS
                patch_at += patch.size
        if dev.type != "cuda":
            return clips, host
        block = host[:4 * words].to(dev, non_blocking=True)
        self._ring[slot][1].record(torch.cuda.current_stream(dev))
        return clips, block

    def launch(self, block, N, T, out, rgb=True):
        """One launch of step_clip_augment_u8 over a packed batch into out [N,T,3,Ho,Wo]."""
        Wo, Ho = self.size
        code = {torch.float32: _capi.F32, torch.bfloat16: _capi.BF16, torch.float16: _capi.F16}[out.dtype]
        m = (ctypes.c_float * 3)(*self.mean)
        sd = (ctypes.c_float * 3)(*self.stds)
        _capi.check(_lib.lib().step_clip_augment_u8(_lib.dptr(block), N, T, Ho, Wo, self.scale, m, sd, 1 if rgb else 0, code, _lib.dptr(out),
                                                    _lib.stream_ptr(out.device)), "step_clip_augment_u8")
        return out

    def apply(self, frames, plans, dtype=torch.bfloat16, out=None, rgb=True):
        """frames: one device uint8 tensor [N,T,Hs,Ws,3] or a list of N per-clip [T,Hs_i,Ws_i,3] device tensors (BGR, as decoded);
        plans: the N AugPlans.  Returns (or fills `out`, whose dtype wins) the clip [N,T,3,Ho,Wo]; rgb applies data/ava.py:335's
        (2,1,0) swap.  One H2D copy of the packed plans, one launch, no host synchronisation."""
        _lib.lib()
        clips, block = self.pack(frames, plans)
        N, T, dev = len(clips), clips[0].shape[0], clips[0].device
        Wo, Ho = self.size
        if out is None:
            out = torch.empty((N, T, 3, Ho, Wo), dtype=dtype, device=dev)
        elif tuple(out.shape) != (N, T, 3, Ho, Wo) or not out.is_contiguous() or out.device != dev:
            raise RuntimeError("step_amd: apply(out=...) wants a contiguous [N,T,3,%d,%d] tensor on the frames' device" % (Ho, Wo))
        return self.launch(block, N, T, out, rgb)


class BaseTransform(_Transform):
    """The evaluation path (data/augmentations.py:601-615): ConvertFromInts(scale), Resize, SubtractMeans, DivideStds."""

    def __init__(self, size=(400, 320), mean=(0, 0, 0), stds=(1, 1, 1), scale=1):
        super().__init__(size, mean, stds, scale)

    def plan(self, shape, tubes=None, proposals=None):
        """Draws nothing: the whole frame, resized."""
        return AugPlan(shape[1], shape[2]), tubes, proposals


class TubeAugmentation(_Transform):
    """The training path (data/augmentations.py:540-586) with the reference's constructor arguments."""

    def __init__(self, size=300, mean=(0, 0, 0), stds=(1, 1, 1), do_flip=False, do_crop=False, do_photometric=False, do_erase=False, scale=1):
        super().__init__(size, mean, stds, scale)
        self.do_flip, self.do_crop, self.do_photometric, self.do_erase = bool(do_flip), bool(do_crop), bool(do_photometric), bool(do_erase)

    def plan(self, shape, tubes, proposals=None):
        """shape = (T, H, W) of the clip's source frames; tubes [n, T, >=4] and proposals [m, T, 4] in percent coordinates.
        Draws from numpy.random in the reference's order and returns (AugPlan, tubes, proposals) -- the tubes and proposals the
        reference's transform returns (percent coordinates of the cropped, mirrored frame).  The inputs are not modified."""
        rnd = np.random
        _, H, W = (int(v) for v in shape)
        p = AugPlan(H, W)
        tubes = np.array(tubes, copy=True)
        proposals = None if proposals is None else np.array(proposals, copy=True)
        if self.do_photometric:
            p.photometric = True
            if rnd.randint(2):
                p.brightness = np.float32(rnd.uniform(-32, 32))
            p.contrast_first = bool(rnd.randint(2))
            if p.contrast_first and rnd.randint(2):
                p.contrast = np.float32(rnd.uniform(0.5, 1.5))
            if rnd.randint(2):
                p.saturation = np.float32(rnd.uniform(0.5, 1.5))
            if rnd.randint(2):
                p.hue = np.float32(rnd.uniform(-18.0, 18.0))
            if not p.contrast_first and rnd.randint(2):
                p.contrast = np.float32(rnd.uniform(0.5, 1.5))
            if rnd.randint(2):
                p.perm = _PERMS[rnd.randint(len(_PERMS))]
        _scale_xy(tubes, W, H, divide=False)
        if proposals is not None:
            _scale_xy(proposals, W, H, divide=False)
        width, height = W, H
        if self.do_crop:
            rect, tubes, proposals = self._crop(width, height, tubes, proposals)
            if rect is not None:
                p.crop = (int(rect[0]), int(rect[1]), int(rect[2] - rect[0]), int(rect[3] - rect[1]))
                width, height = p.crop[2], p.crop[3]
        if self.do_flip:
            src, tubes = tubes, tubes.copy()
            psrc, proposals = proposals, (None if proposals is None else proposals.copy())
            if rnd.randint(2):
                p.mirror = True
                real = np.sum(src[:, :, :4], axis=2) > 0                       # (zero-padded boxes stay where they are)
                tubes[:, :, 0] = np.where(real, width - src[:, :, 2], src[:, :, 0])
                tubes[:, :, 2] = np.where(real, width - src[:, :, 0], src[:, :, 2])
                if psrc is not None:
                    proposals[:, :, 0] = width - psrc[:, :, 2]
                    proposals[:, :, 2] = width - psrc[:, :, 0]
        if self.do_erase and rnd.randint(2):
            lo, hi = _NOISE_RANGE[self.scale]
            for box in _mid_boxes(tubes):
                x1, y1, x2, y2 = self._erase_region(box)
                p.rects.append((x1, y1, x2, y2))
                p.patches.append(np.random.uniform(lo, hi, (y2 - y1, x2 - x1, 3)).astype(np.float32))
        _scale_xy(tubes, width, height, divide=True)
        if proposals is not None:
            _scale_xy(proposals, width, height, divide=True)
        p.check()
        return p, tubes, proposals

    @staticmethod
    def _crop(width, height, tubes, proposals):
        """RandomSampleCrop (data/augmentations.py:308-423): returns (rect or None, tubes, proposals)."""
        rnd = np.random
        boxes = _mid_boxes(tubes)
        while True:
            min_iou = _CROP_MIN_IOU[rnd.randint(len(_CROP_MIN_IOU))]            # (random.choice over the 7 modes draws the same randint)
            if min_iou is None:
                return None, tubes, proposals
            for _ in range(50):
                w = rnd.uniform(0.3 * width, width)
                h = rnd.uniform(0.3 * height, height)
                if h / w < 0.5 or h / w > 2:
                    continue
                left = rnd.uniform(width - w)                                   # (one argument: low = width - w, high = 1.0)
                top = rnd.uniform(height - h)
                rect = np.array([int(left), int(top), int(left + w), int(top + h)])
                hi = np.minimum(boxes[:, 2:], rect[2:])
                lo = np.maximum(boxes[:, :2], rect[:2])
                side = np.clip(hi - lo, a_min=0, a_max=np.inf)
                inter = side[:, 0] * side[:, 1]
                area_b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
                area_r = (rect[2] - rect[0]) * (rect[3] - rect[1])
                overlap = inter / (area_b + area_r - inter)
                if overlap.min() < min_iou:                                     # (no mode of the reference sets a maximum)
                    continue
                centre = (boxes[:, :2] + boxes[:, 2:]) / 2.0
                keep = (rect[0] < centre[:, 0]) * (rect[1] < centre[:, 1]) * ((rect[2] > centre[:, 0]) * (rect[3] > centre[:, 1]))
                if not keep.any():
                    continue
                kept = tubes[keep, :, :].copy()
                _shift_into(kept, rect)
                kept[:, :, :4] = np.maximum(kept[:, :, :4], 0.)
                if proposals is not None:
                    proposals = proposals.copy()
                    _shift_into(proposals, rect)
                    proposals = _valid_tubes(proposals, width=w, height=h)
                return rect, kept, proposals

    @staticmethod
    def _erase_region(box, sl=0.02, sh=0.2, r1=0.3, r2=10 / 3.):
        """RandomErase.get_region (data/augmentations.py:291-303): area share in [sl, sh], aspect in [r1, r2], inside the box."""
        rnd = np.random
        x1, y1, x2, y2 = box
        S = (x2 - x1) * (y2 - y1)
        while True:
            Se = rnd.uniform(sl, sh) * S
            re = rnd.uniform(r1, r2)
            He = np.sqrt(Se * re)
            We = np.sqrt(Se / re)
            xe = rnd.uniform(x1, x2 - We)
            ye = rnd.uniform(y1, y2 - He)
            if xe + We <= x2 and ye + He <= y2:
                return int(xe), int(ye), int(xe + We), int(ye + He)


class DeviceTubeAugmentation(_Transform):
    """TubeAugmentation with the DECISIONS made on the device too (include/step_amd.h: step_augment_plan): the constructor arguments of
    TubeAugmentation plus `rng`, a step_amd.DeviceRNG.  `.apply()` is the planner, the noise fill and step_clip_augment_u8 on the current
    stream -- three launches, two offsets of `rng`, no copy and no host synchronisation, so the calls can be recorded in a graph and every
    replay draws anew.  Besides the clip it writes the transformed ground truths, the `gt` / `gt_count` step_select_train reads.  Same
    rule as TubeAugmentation.plan, other draws (the device generator's, not numpy's).  With `tubes=` the planner transforms the clips'
    detector proposals as well (step_augment_plan_tubes: the same launches and offsets) into padded slots with a device-side count."""

    def __init__(self, size=300, mean=(0, 0, 0), stds=(1, 1, 1), do_flip=False, do_crop=False, do_photometric=False, do_erase=False, scale=1,
                 rng=None):
        super().__init__(size, mean, stds, scale)
        self.rng = rng                                       # (None: bound later by the workload whose generator it shares)
        self.do_flip, self.do_crop, self.do_photometric, self.do_erase = bool(do_flip), bool(do_crop), bool(do_photometric), bool(do_erase)
        self.switches = (1 if self.do_flip else 0) | (2 if self.do_crop else 0) | (4 if self.do_photometric else 0) | (8 if self.do_erase else 0)
        self._static = None                                  # (key, block, max_hw): one block per (N, Gmax, largest frame)
        self._frames = None                                  # (key, src [N] int64, dims [N,2] int32) of the frame buffers last seen

    def _block(self, N, Gmax, max_hw, dev):
        key = (N, Gmax, max_hw, dev)
        if self._static is None or self._static[0] != key:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("step_amd: DeviceTubeAugmentation builds its plan block on the first apply() of a batch shape; run apply() once before capturing")
            nbytes = _lib.lib().step_augment_plan_bytes(N, Gmax, max_hw, None)
            if nbytes == 0:
                raise RuntimeError("step_amd: no plan block for N=%d, Gmax=%d, frames of %d pixels" % (N, Gmax, max_hw))
            self._static = (key, torch.zeros(nbytes, dtype=torch.uint8, device=dev))
        return self._static[1]

    def _sources(self, clips, dev):
        """the clips' addresses and sizes ON THE DEVICE: uploaded when other frame buffers are handed in than the last time (the stage
        buffer of a captured step never changes), so not inside a capture"""
        key = tuple((c.data_ptr(), c.shape[1], c.shape[2]) for c in clips)
        if self._frames is None or self._frames[0] != key:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("step_amd: DeviceTubeAugmentation cannot take new frame buffers inside a graph capture (run apply() on them once before)")
            src = np.array([k[0] for k in key], np.uint64).view(np.int64)
            dims = np.array([[k[1], k[2]] for k in key], np.int32)
            self._frames = (key, torch.from_numpy(src).to(dev), torch.from_numpy(dims).to(dev))
        return self._frames[1], self._frames[2]

    def apply(self, frames, gt, gt_count, out=None, gt_out=None, gt_count_out=None, dtype=torch.bfloat16, rgb=True, tubes=None, tube_count=None,
              fill=None, tubes_out=None, tube_count_out=None):
        """frames: one device uint8 tensor [N,T,Hs,Ws,3] or a list of N per-clip [T,Hs_i,Ws_i,3] device tensors (BGR); gt [N,Gmax,F,4+NC]
        float32 percent boxes + labels (an all-zero box pads a tube) and gt_count [N] int32, on the device.  Returns (clip [N,T,3,Ho,Wo],
        gt_out [N,Gmax,F,4+NC] in pixels of the network's resolution, kept tubes first, gt_count_out [N]); `out`, `gt_out`,
        `gt_count_out` are filled when given (out's dtype wins).
        tubes [N,Pmax,Tp,4] float32 percent boxes with tube_count [N] int32: the clips' proposals, transformed with the frames; fill [n,4]
        float32 percent boxes stands in, untransformed, for a clip without any (the anchor grid).  The call then returns two more tensors:
        tubes_out [N,Pmax,Tp,4] in pixels of the network's resolution -- the first tube_count_out[n] slots of a clip real, the others the
        whole frame -- and tube_count_out [N] int32 (both filled when given)."""
        L = _lib.lib()
        clips = list(frames.unbind(0)) if torch.is_tensor(frames) else list(frames)
        N = len(clips)
        if N == 0:
            raise RuntimeError("step_amd: apply() wants at least one clip")
        T, dev = clips[0].shape[0], clips[0].device
        for c in clips:
            if c.dtype != torch.uint8 or c.dim() != 4 or c.shape[-1] != 3 or not c.is_contiguous() or c.device != dev or c.shape[0] != T:
                raise RuntimeError("step_amd: apply() expects contiguous uint8 clips [T,H,W,3] of one length on one device")
        if gt.dim() != 4 or gt.shape[0] != N or gt.shape[3] < 4 or gt.dtype != torch.float32 or not gt.is_contiguous() or gt.device != dev:
            raise RuntimeError("step_amd: apply() wants gt as a contiguous float32 [N,Gmax,F,4+NC] tensor on the frames' device")
        if tuple(gt_count.shape) != (N,) or gt_count.dtype != torch.int32 or gt_count.device != dev:
            raise RuntimeError("step_amd: apply() wants gt_count as an int32 [N] tensor on the frames' device")
        if self.rng is None:
            raise RuntimeError("step_amd: DeviceTubeAugmentation needs rng, a step_amd.DeviceRNG")
        if self.rng.device.type != dev.type or self.rng.device.index not in (None, dev.index):
            raise RuntimeError("step_amd: the generator lives on %s, the frames on %s" % (self.rng.device, dev))
        Gmax, F, NC = gt.shape[1], gt.shape[2], gt.shape[3] - 4
        Wo, Ho = self.size
        if out is None:
            out = torch.empty((N, T, 3, Ho, Wo), dtype=dtype, device=dev)
        elif tuple(out.shape) != (N, T, 3, Ho, Wo) or not out.is_contiguous() or out.device != dev:
            raise RuntimeError("step_amd: apply(out=...) wants a contiguous [N,T,3,%d,%d] tensor on the frames' device" % (Ho, Wo))
        if gt_out is None:
            gt_out = torch.empty_like(gt)
        elif gt_out.shape != gt.shape or gt_out.dtype != torch.float32 or not gt_out.is_contiguous() or gt_out.device != dev:
            raise RuntimeError("step_amd: apply(gt_out=...) wants a contiguous float32 tensor of gt's shape on the frames' device")
        if gt_count_out is None:
            gt_count_out = torch.empty_like(gt_count)
        elif tuple(gt_count_out.shape) != (N,) or gt_count_out.dtype != torch.int32 or gt_count_out.device != dev:
            raise RuntimeError("step_amd: apply(gt_count_out=...) wants an int32 [N] tensor on the frames' device")
        Pmax = Tp = n_fill = 0
        if tubes is not None:
            if tubes.dim() != 4 or tubes.shape[0] != N or tubes.shape[3] != 4 or tubes.dtype != torch.float32 or not tubes.is_contiguous() or tubes.device != dev:
                raise RuntimeError("step_amd: apply() wants tubes as a contiguous float32 [N,Pmax,Tp,4] tensor on the frames' device")
            if tube_count is None or tuple(tube_count.shape) != (N,) or tube_count.dtype != torch.int32 or tube_count.device != dev:
                raise RuntimeError("step_amd: apply() wants tube_count as an int32 [N] tensor on the frames' device")
            if fill is not None and (fill.dim() != 2 or fill.shape[1] != 4 or fill.dtype != torch.float32 or not fill.is_contiguous() or fill.device != dev):
                raise RuntimeError("step_amd: apply() wants fill as a contiguous float32 [n,4] tensor on the frames' device")
            Pmax, Tp, n_fill = tubes.shape[1], tubes.shape[2], (0 if fill is None else fill.shape[0])
            if tubes_out is None:
                tubes_out = torch.empty_like(tubes)
            elif tubes_out.shape != tubes.shape or tubes_out.dtype != torch.float32 or not tubes_out.is_contiguous() or tubes_out.device != dev:
                raise RuntimeError("step_amd: apply(tubes_out=...) wants a contiguous float32 tensor of tubes' shape on the frames' device")
            if tube_count_out is None:
                tube_count_out = torch.empty_like(tube_count)
            elif tuple(tube_count_out.shape) != (N,) or tube_count_out.dtype != torch.int32 or tube_count_out.device != dev:
                raise RuntimeError("step_amd: apply(tube_count_out=...) wants an int32 [N] tensor on the frames' device")
        elif tube_count is not None or fill is not None or tubes_out is not None or tube_count_out is not None:
            raise RuntimeError("step_amd: apply() takes tube_count, fill, tubes_out and tube_count_out only with tubes")
        max_hw = max(c.shape[1] * c.shape[2] for c in clips)
        block = self._block(N, Gmax, max_hw, dev)
        src, dims = self._sources(clips, dev)
        _capi.check(L.step_augment_plan_tubes(_lib.dptr(src), _lib.dptr(dims), _lib.dptr(gt), _lib.dptr(gt_count), N, Gmax, F, NC, self.switches,
                                              self.scale, Wo, Ho, max_hw, _lib.dptr(self.rng.state), _lib.dptr(block), _lib.dptr(gt_out),
                                              _lib.dptr(gt_count_out), _lib.dptr(tubes), _lib.dptr(tube_count), Pmax, Tp, _lib.dptr(fill), n_fill,
                                              _lib.dptr(tubes_out), _lib.dptr(tube_count_out), _lib.stream_ptr(dev)), "step_augment_plan_tubes")
        self.launch(block, N, T, out, rgb)
        if tubes is not None:
            return out, gt_out, gt_count_out, tubes_out, tube_count_out
        return out, gt_out, gt_count_out

    def last_block(self):
        """the plan block of the last apply() (a uint8 device tensor in the layout of include/step_amd.h), for inspection"""
        if self._static is None:
            raise RuntimeError("step_amd: no apply() yet")
        return self._static[1]
