"""Cases for the device-drawn clip augmentation (step_augment_plan, step_amd.DeviceTubeAugmentation), driven on the host interpreter by
tests/test_emul_augplan.py and on the real library by tests/test_gpu_augplan.py.

The reference of every kernel comparison is `restate_clip` below: the rule of include/step_amd.h ("The rule, per clip") written again in
plain Python on numpy scalars, every operand cast explicitly so that the arithmetic does not depend on numpy's promotion rules.  Its words
come from a `words(seed, offset, first_blk, n_blk)` function: tests/dropout_cases.philox_words, which case_words_are_the_librarys holds
against step_rng_words on the very blocks the rule addresses.  Blocks, patches, gt_out and gt_count_out are compared for EQUALITY, floats as
bits: the rule is a fixed sequence of IEEE operations, there is nothing to tolerate.

The restatement evaluates the trials ONE AFTER THE OTHER, as the host rule does, and records every draw it consumed; `host_plan` then runs
TubeAugmentation.plan with numpy.random.uniform / randint replaced for the call by a feeder that replays those draws, which ties the
device rule to the host rule that tests/golden/augment_golden.npz pins.  Two things the host form cannot do are left out of that comparison
and say so: a case that hit one of the two caps (the host loops on), and a clip without tubes whose crop draws a mode other than None
(numpy raises on the minimum over no boxes; the device rule rejects the trial because no box is kept).

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda")."""
import ctypes
import math

import numpy as np

from step_amd.augment import AugPlan, TubeAugmentation
from tests import augment_cases as AC
from tests.dropout_cases import philox_words

f32, f64, u64 = np.float32, np.float64, np.uint64
E_SHAPE, E_NULL, E_UNSUPPORTED, E_ALIGN = -2, -3, -4, -5
FLIP, CROP, PHOTO, ERASE = 1, 2, 4, 8
ALL = FLIP | CROP | PHOTO | ERASE
COMBOS = (ALL, FLIP, CROP, PHOTO, ERASE, 0)
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
MIN_IOU = (None, 0.1, 0.3, 0.5, 0.7, 0.9, float("-inf"))
NOISE = {0: (0.0, 255.0), 1: (0.0, 1.0), 2: (-1.0, 1.0)}
CROP_ROUNDS, CROP_TRIALS, ERASE_TRIALS = 16, 50, 64

# ---- the inputs: the smallest that still take every branch -----------------------------------------------------------------------------
DIMS = ((24, 32), (40, 28), (33, 47))                       # (Hs, Ws) of the three clips
T, GMAX, F, NC = 3, 4, 3, 5
COUNTS = (2, 4, 0)
WN, HN = 20, 12
SCALE = 2
MEAN, STDS = (0.1, 0.2, 0.3), (0.9, 1.1, 1.2)
SEEDS = (1, 2, 3, 5, 8, 13, 0x1_0000_0007, 0xFFFF_FFFF_FFFF_FFF1)
OFFSETS = (0, 1, 2, 7, 100, 0xFFFF_FFFE, 0xFFFF_FFFF, 1 << 40)
PAIRS = tuple((s, o) for s in SEEDS for o in OFFSETS)       # 64


def make_gt(sliver=False):
    """gt [3,GMAX,F,4+NC] percent boxes + labels and gt_count.  Clip 1 holds a tube whose first frame is padding and a thin box, 3 px wide
    in its 28 px frame (so that get_region rejects trials); slots past a clip's count hold other numbers, which the kernel must not use.
    sliver: the thin box is 0.02 px wide instead -- every get_region trial is then rejected (see case_caps)."""
    rs = np.random.RandomState(11)
    gt = rs.uniform(0.05, 0.6, (3, GMAX, F, 4 + NC)).astype(f32)
    gt[..., 2:4] = gt[..., 0:2] + rs.uniform(0.2, 0.35, (3, GMAX, F, 2)).astype(f32)
    gt[..., 4:] = (rs.rand(3, GMAX, F, NC) < 0.4)
    gt[1, 1, 0, :] = 0                                                          # a padding frame (labels too, as the loader pads)
    wide = 0.02 if sliver else 3.0
    for f in range(F):
        gt[1, 2, f, :4] = (0.5, 0.1 + 0.01 * f, 0.5 + wide / 28.0, 0.9)
    return gt, np.asarray(COUNTS, np.int32)


def cap_words_of(max_hw):
    """the header's bound: 3 (floor(0.2 A + 2 sqrt(2 A / 3) + 1) + 2)"""
    return 3 * (int(0.2 * max_hw + 2.0 * math.sqrt(2.0 * max_hw / 3.0) + 1.0) + 2)


def layout(N, Gmax, max_hw):
    cap = cap_words_of(max_hw)
    rec = 16 * N + 6 * Gmax * N
    words = rec + 4 + N * Gmax * cap
    return dict(cap=cap, rec=rec, patch_base=rec + 4, words=(words + 3) // 4 * 4)


MAX_HW = max(h * w for h, w in DIMS)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
class Draws:
    """u(phase, k) of clip n at (seed, offset), fetched in runs of 64 blocks; .log lists what the rule consumed, in order"""

    def __init__(self, words, seed, offset, n):
        self.words, self.seed, self.offset, self.n, self.cache, self.log = words, seed, offset, n, {}, []

    def u(self, phase, k):
        key = (phase, k >> 6)
        if key not in self.cache:
            w = self.words(self.seed, self.offset, (self.n << 20) | (phase << 16) | (k & ~63), 64)
            self.cache[key] = ((w[:, 0] << u64(21)) | (w[:, 1] >> u64(11))).astype(f64) * 2.0 ** -53
        return float(self.cache[key][k & 63])

    def randint(self, m, phase, k):
        u = self.u(phase, k)
        self.log.append(("randint", m, None, u))
        return min(int(math.floor(u * m)), m - 1)

    def uniform(self, a, b, phase, k):
        u = self.u(phase, k)
        a, b = float(a), float(b)
        self.log.append(("uniform", a, b, u))
        return a + (b - a) * u

    def uniform1(self, a, phase, k):
        u = self.u(phase, k)
        a = float(a)
        self.log.append(("uniform", a, 1.0, u))
        return a + (1.0 - a) * u


def _box(q, W, H, rect, mirror, width):
    """box q (percent) in pixels of the cropped, mirrored frame, fp32 operation by operation"""
    b = [f32(q[0]) * f32(W), f32(q[1]) * f32(H), f32(q[2]) * f32(W), f32(q[3]) * f32(H)]
    z = f32(0)
    if rect is not None:
        x0, y0, x1, y1 = (f32(v) for v in rect)
        b = [max(z, max(x0, b[0]) - x0), max(z, max(y0, b[1]) - y0), max(z, min(x1, b[2]) - x0), max(z, min(y1, b[3]) - y0)]
    if mirror and ((b[0] + b[1]) + b[2]) + b[3] > 0:
        b[0], b[2] = f32(width) - b[2], f32(width) - b[0]
    return b


def restate_clip(n, dims, gt, G, switches, Wn, Hn, cap, seed, offset, words=philox_words, seen=None):
    """-> dict: the step_aug_clip fields, rects, K, kept, tubes_pct [K,F,4+NC] (the host transform's output), gt_rows [K,F,4+NC], the draw log,
    crop_cap / erase_cap / dropped, and `seen` (a set of the branches taken) updated"""
    seen = set() if seen is None else seen
    H, W = dims
    Fr, E = gt.shape[1], gt.shape[2]
    mid = Fr // 2
    d = Draws(words, seed, offset, n)
    r = dict(Hs=H, Ws=W, flags=0, perm=(0, 1, 2), par=[f32(0)] * 4, crop=(0, 0, W, H), rects=[], crop_cap=False, erase_cap=False, dropped=0,
             mode_first=None)
    with np.errstate(all="ignore"):
        if switches & PHOTO:
            r["flags"] |= AC_F["photometric"]
            def param(name, slot, coin_k, a, b):
                on = d.randint(2, 0, coin_k)
                seen.add((name, bool(on)))
                if on:
                    r["flags"] |= AC_F[name]
                    r["par"][slot] = f32(d.uniform(a, b, 0, coin_k + 1))
            param("brightness", 0, 0, -32, 32)
            first = d.randint(2, 0, 2)
            seen.add(("contrast_first", bool(first)))
            if first:
                r["flags"] |= AC_F["contrast_first"]
                param("contrast", 1, 3, 0.5, 1.5)
            param("saturation", 2, 5, 0.5, 1.5)
            param("hue", 3, 7, -18.0, 18.0)
            if not first:
                param("contrast", 1, 9, 0.5, 1.5)
            on = d.randint(2, 0, 11)
            seen.add(("perm", bool(on)))
            if on:
                r["perm"] = PERMS[d.randint(6, 0, 12)]
        rect, kept = None, list(range(G))
        if switches & CROP:
            boxes = [_box(gt[g, mid], W, H, None, False, W) for g in range(G)]
            done = False
            for rnd in range(CROP_ROUNDS):
                mode = d.randint(7, 1, CROP_ROUNDS * CROP_TRIALS * 4 + rnd)
                if rnd == 0:
                    r["mode_first"] = mode
                if mode == 0:
                    seen.add("mode_none")
                    done = True
                    break
                for t in range(CROP_TRIALS):
                    kb = (rnd * CROP_TRIALS + t) * 4
                    w = d.uniform(0.3 * W, W, 1, kb)
                    h = d.uniform(0.3 * H, H, 1, kb + 1)
                    if h / w < 0.5 or h / w > 2:
                        seen.add("aspect_continue")
                        continue
                    left = d.uniform1(W - w, 1, kb + 2)
                    top = d.uniform1(H - h, 1, kb + 3)
                    rc = (int(left), int(top), int(left + w), int(top + h))
                    if not (rc[0] >= 0 and rc[1] >= 0 and rc[2] > rc[0] and rc[3] > rc[1] and rc[2] <= W and rc[3] <= H):
                        seen.add("crop_outside")
                        continue
                    area_r = f64((rc[2] - rc[0]) * (rc[3] - rc[1]))
                    ov, keep = [], []
                    for b in boxes:
                        bd = [f64(v) for v in b]
                        sx = max(f64(0), min(f64(rc[2]), bd[2]) - max(f64(rc[0]), bd[0]))
                        sy = max(f64(0), min(f64(rc[3]), bd[3]) - max(f64(rc[1]), bd[1]))
                        inter = sx * sy
                        area_b = (b[2] - b[0]) * (b[3] - b[1])                                  # fp32
                        ov.append(inter / ((f64(area_b) + area_r) - inter))
                        cx, cy = (b[0] + b[2]) / f32(2), (b[1] + b[3]) / f32(2)
                        keep.append(bool(rc[0] < f64(cx) and rc[1] < f64(cy) and rc[2] > f64(cx) and rc[3] > f64(cy)))
                    if ov and not any(math.isnan(v) for v in ov) and min(ov) < MIN_IOU[mode]:
                        continue
                    if not any(keep):
                        continue
                    rect, kept = rc, [g for g in range(G) if keep[g]]
                    seen.add("crop_taken")
                    if len(kept) < G:
                        seen.add("crop_drops_tube")
                    done = True
                    break
                if done:
                    break
            if not done:
                r["crop_cap"] = True
        width, height = (W, H) if rect is None else (rect[2] - rect[0], rect[3] - rect[1])
        if rect is not None:
            r["crop"] = (rect[0], rect[1], width, height)
        mirror = bool(switches & FLIP) and bool(d.randint(2, 2, 0))
        if switches & FLIP:
            seen.add(("mirror", mirror))
        if mirror:
            r["flags"] |= AC_F["mirror"]
        r["erase_coin"] = bool(switches & ERASE) and bool(d.randint(2, 2, 1))
        if r["erase_coin"]:
            for j, g in enumerate(kept):
                x1, y1, x2, y2 = _box(gt[g, mid], W, H, rect, mirror, width)
                S = (x2 - x1) * (y2 - y1)
                got = None
                for t in range(ERASE_TRIALS):
                    kb = (j * ERASE_TRIALS + t) * 4
                    Se = f32(d.uniform(0.02, 0.2, 3, kb)) * S
                    re = f32(d.uniform(0.3, 10 / 3., 3, kb + 1))
                    He, We = np.sqrt(Se * re), np.sqrt(Se / re)
                    assert He.dtype == f32 and We.dtype == f32
                    xe = d.uniform(x1, x2 - We, 3, kb + 2)
                    ye = d.uniform(y1, y2 - He, 3, kb + 3)
                    xr, yr = f32(xe) + We, f32(ye) + He
                    if xr <= x2 and yr <= y2:
                        got = (int(xe), int(ye), int(xr), int(yr))
                        break
                    seen.add("erase_reject")
                if got is None:
                    r["erase_cap"] = True
                    continue
                a, b_, c, e = got
                if not (a >= 0 and b_ >= 0 and a <= c and b_ <= e and c <= width and e <= height and (c - a) * (e - b_) * 3 <= cap):
                    r["dropped"] += 1
                    continue
                r["rects"].append(got)
            if len(r["rects"]) >= 2:
                seen.add("erase_2plus")
        K = len(kept)
        pct = np.zeros((K, Fr, E), f32)
        rows = np.zeros((K, Fr, E), f32)
        for j, g in enumerate(kept):
            for f in range(Fr):
                b = _box(gt[g, f], W, H, rect, mirror, width)
                p = [b[0] / f32(width), b[1] / f32(height), b[2] / f32(width), b[3] / f32(height)]
                pct[j, f, :4] = p
                pct[j, f, 4:] = gt[g, f, 4:]
                rows[j, f, :4] = [min(f32(1), max(f32(0), p[c])) * f32(Hn if c & 1 else Wn) for c in range(4)]
                rows[j, f, 4:] = gt[g, f, 4:]
    r.update(K=K, kept=kept, tubes_pct=pct, gt_rows=rows, log=d.log, mirror=mirror)
    return r


AC_F = dict(mirror=1, photometric=2, brightness=4, contrast=8, contrast_first=16, saturation=32, hue=64)       # include/step_amd.h


def noise(seed, offset, slot, n_elem, scale, words=philox_words):
    lo, hi = NOISE[scale]
    w = words(seed, offset + 1, slot << 20, (n_elem + 3) // 4).reshape(-1)[:n_elem]
    return (lo + (hi - lo) * ((w >> u64(8)).astype(f64) * 2.0 ** -24)).astype(f32)


def restate(dims, gt, counts, switches, seed, offset, scale=SCALE, Wn=WN, Hn=HN, max_hw=None, words=philox_words, seen=None):
    """-> (block as int32 words with src = 0, [(start, stop)] of the patch words in use, gt_out, gt_count_out, per-clip records)"""
    N, Gmax = gt.shape[0], gt.shape[1]
    L = layout(N, Gmax, max_hw or max(h * w for h, w in dims))
    blk = np.zeros(L["words"], np.int32)
    fl = blk.view(f32)
    gt_out = np.zeros(gt.shape, f32)
    cnt_out = np.zeros(N, np.int32)
    used, recs = [], []
    for n in range(N):
        G = min(max(int(counts[n]), 0), Gmax)
        r = restate_clip(n, dims[n], gt[n], G, switches, Wn, Hn, L["cap"], seed, offset, words, seen)
        o = 16 * n
        rect_off = 16 * N + 6 * Gmax * n
        pm = r["perm"]
        blk[o + 2:o + 10] = (r["Hs"], r["Ws"]) + tuple(r["crop"]) + (r["flags"], pm[0] | pm[1] << 2 | pm[2] << 4)
        fl[o + 10:o + 14] = r["par"]
        blk[o + 14:o + 16] = (len(r["rects"]), rect_off)
        r["patches"] = []
        for k, rc in enumerate(r["rects"]):
            at = L["patch_base"] + (n * Gmax + k) * L["cap"]
            blk[rect_off + 6 * k:rect_off + 6 * k + 6] = tuple(rc) + (at, 0)
            ne = (rc[3] - rc[1]) * (rc[2] - rc[0]) * 3
            fl[at:at + ne] = noise(seed, offset, n * Gmax + k, ne, scale, words)
            r["patches"].append(fl[at:at + ne].reshape(rc[3] - rc[1], rc[2] - rc[0], 3).copy())
            used.append((at, at + ne))
        gt_out[n, :r["K"]] = r["gt_rows"]
        cnt_out[n] = r["K"]
        recs.append(r)
    if N:
        blk[L["rec"]:L["rec"] + 2] = np.array([offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF], np.uint32).view(np.int32)
    return blk, used, gt_out, cnt_out, recs


_RESTATED = {}


def restated(switches, seed, offset, sliver=False):
    """the restatement of the standard inputs, once per session (shared by the backends and the cases)"""
    key = (switches, seed, offset, sliver)
    if key not in _RESTATED:
        gt, cnt = make_gt(sliver)
        _RESTATED[key] = restate(DIMS, gt, cnt, switches, seed, offset)
    return _RESTATED[key]


# ---- driving the C ABI -----------------------------------------------------------------------------------------------------------------
def _state(bk, seed, offset):
    return bk.dev(np.array([seed, offset], u64).view(np.int64))


def _read_state(st):
    s = st.get().view(u64)
    return int(s[0]), int(s[1])


def _addr(ptr):
    return 0 if ptr is None else (ptr.value if isinstance(ptr, ctypes.c_void_p) else int(ptr))


class Call:
    """the device buffers of one batch, reusable over many calls of step_augment_plan"""

    def __init__(self, bk, dims, gt, counts, frames=None, max_hw=None):
        self.bk, self.N, self.Gmax, self.F, self.NC = bk, gt.shape[0], gt.shape[1], gt.shape[2], gt.shape[3] - 4
        self.max_hw = max_hw or max(h * w for h, w in dims)
        self.L = layout(self.N, self.Gmax, self.max_hw)
        cap = ctypes.c_int()
        nbytes = bk.lib.step_augment_plan_bytes(self.N, self.Gmax, self.max_hw, ctypes.byref(cap))
        assert (nbytes, cap.value) == (4 * self.L["words"], self.L["cap"]), (nbytes, cap.value, self.L)
        self.frames = None if frames is None else [bk.dev(f) for f in frames]
        src = np.array([0x1000 * (n + 1) for n in range(self.N)] if frames is None else [_addr(f.ptr) for f in self.frames], u64)
        self.src_host = src
        self.src, self.dims = bk.dev(src.view(np.int64)), bk.dev(np.asarray(dims, np.int32))
        self.gt, self.cnt = bk.dev(gt), bk.dev(np.asarray(counts, np.int32))
        self.fresh()

    def fresh(self):
        self.block = self.bk.dev(np.full(self.L["words"], 0x7A7A7A7A, np.int32))
        self.gt_out = self.bk.dev(np.full((self.N, self.Gmax, self.F, 4 + self.NC), 7, f32))
        self.cnt_out = self.bk.dev(np.full(self.N, 7, np.int32))

    def untouched(self):
        return bool(np.all(self.block.get() == 0x7A7A7A7A) and np.all(self.gt_out.get() == 7) and np.all(self.cnt_out.get() == 7))

    def run(self, st, switches=ALL, scale=SCALE, Wn=WN, Hn=HN, **o):
        a = dict(src=self.src.ptr, dims=self.dims.ptr, gt=self.gt.ptr, cnt=self.cnt.ptr, N=self.N, Gmax=self.Gmax, F=self.F, NC=self.NC,
                 switches=switches, scale=scale, Wn=Wn, Hn=Hn, max_hw=self.max_hw, rng=st.ptr, block=self.block.ptr, gt_out=self.gt_out.ptr,
                 cnt_out=self.cnt_out.ptr)
        a.update(o)
        return self.bk.lib.step_augment_plan(a["src"], a["dims"], a["gt"], a["cnt"], a["N"], a["Gmax"], a["F"], a["NC"], a["switches"], a["scale"],
                                             a["Wn"], a["Hn"], a["max_hw"], a["rng"], a["block"], a["gt_out"], a["cnt_out"], self.bk.stream)


def same_outputs(call, want, what):
    blk, used, gt_out, cnt_out, _ = want
    got = call.block.get().view(np.int32).copy()
    N = call.N
    assert np.array_equal(got[:16 * N].view(u64).reshape(N, 8)[:, 0], call.src_host), (what, "src")
    got[:16 * N].reshape(N, 16)[:, :2] = 0
    head = call.L["patch_base"]
    bad = np.flatnonzero(got[:head] != blk[:head])
    assert bad.size == 0, (what, "block words", bad[:8].tolist(), got[bad[:8]].tolist(), blk[bad[:8]].tolist())
    for a, b in used:
        assert np.array_equal(got[a:b], blk[a:b]), (what, "patch at", a)
    assert np.array_equal(call.gt_out.get().view(np.int32), gt_out.view(np.int32)), (what, "gt_out")
    assert np.array_equal(call.cnt_out.get(), cnt_out), (what, "gt_count_out", call.cnt_out.get(), cnt_out)


# ---- the host form, fed with the device's draws ------------------------------------------------------------------------------------------
class _Feeder:
    def __init__(self, log, patches):
        self.log, self.at, self.patches, self.pk = log, 0, patches, 0

    def _next(self, kind):
        assert self.at < len(self.log), "the host rule draws more than the restatement consumed"
        rec = self.log[self.at]
        self.at += 1
        assert rec[0] == kind, (self.at, rec, kind)
        return rec

    def randint(self, m):
        _, want_m, _, u = self._next("randint")
        assert want_m == m, (want_m, m)
        return min(int(math.floor(u * m)), m - 1)

    def uniform(self, a=0.0, b=1.0, size=None):
        if size is not None:
            p = self.patches[self.pk]
            self.pk += 1
            assert tuple(size) == p.shape, (size, p.shape)
            return p.astype(f64)
        _, wa, wb, u = self._next("uniform")
        a, b = float(a), float(b)
        assert (a, b) == (wa, wb), ("the host rule draws from another interval", (a, b), (wa, wb))
        return a + (b - a) * u


def host_plan(aug, dims, tubes, rec):
    """TubeAugmentation.plan with numpy.random.uniform / randint replaced FOR THE CALL by the feeder -> (AugPlan, tubes)"""
    feed = _Feeder(rec["log"], rec["patches"])
    saved = (np.random.uniform, np.random.randint)
    np.random.uniform, np.random.randint = feed.uniform, feed.randint
    try:
        plan, out, _ = aug.plan((T, dims[0], dims[1]), tubes)
    finally:
        np.random.uniform, np.random.randint = saved
    assert feed.at == len(rec["log"]) and feed.pk == len(rec["patches"]), "the host rule consumed fewer draws than the restatement"
    return plan, out


def plan_of(rec):
    """the AugPlan a restated (or read back) clip record describes"""
    p = AugPlan(rec["Hs"], rec["Ws"])
    fl = rec["flags"]
    p.crop, p.mirror, p.photometric, p.perm = tuple(rec["crop"]), bool(fl & 1), bool(fl & 2), tuple(rec["perm"])
    p.contrast_first = bool(fl & 16)
    p.brightness = f32(rec["par"][0]) if fl & 4 else None
    p.contrast = f32(rec["par"][1]) if fl & 8 else None
    p.saturation = f32(rec["par"][2]) if fl & 32 else None
    p.hue = f32(rec["par"][3]) if fl & 64 else None
    p.rects, p.patches = [tuple(r) for r in rec["rects"]], list(rec["patches"])
    return p


def read_block(words, N, Gmax):
    """the clip records a block holds (as restate_clip names them), patches included"""
    fl = words.view(f32)
    out = []
    for n in range(N):
        c = words[16 * n:16 * n + 16]
        pm = int(c[9])
        r = dict(Hs=int(c[2]), Ws=int(c[3]), crop=tuple(int(v) for v in c[4:8]), flags=int(c[8]), perm=(pm & 3, pm >> 2 & 3, pm >> 4 & 3),
                 par=[f32(v) for v in fl[16 * n + 10:16 * n + 14]], rects=[], patches=[], rect_off=int(c[15]), patch_offs=[])
        for k in range(int(c[14])):
            x1, y1, x2, y2, at, _ = (int(v) for v in words[r["rect_off"] + 6 * k:r["rect_off"] + 6 * k + 6])
            r["rects"].append((x1, y1, x2, y2))
            r["patch_offs"].append(at)
            r["patches"].append(fl[at:at + (y2 - y1) * (x2 - x1) * 3].reshape(y2 - y1, x2 - x1, 3).copy())
        out.append(r)
    return out


def block_is_safe(words, N, Gmax, dims, L):
    """what step_clip_augment_u8 trusts: crops inside frames, rectangles inside crops, patches inside their slots"""
    for n, r in enumerate(read_block(words, N, Gmax)):
        x, y, w, h = r["crop"]
        assert (r["Hs"], r["Ws"]) == tuple(dims[n]) and 0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= r["Ws"] and y + h <= r["Hs"], (n, r["crop"])
        assert len(r["rects"]) <= Gmax and r["rect_off"] == 16 * N + 6 * Gmax * n
        for k, ((x1, y1, x2, y2), at) in enumerate(zip(r["rects"], r["patch_offs"])):
            assert 0 <= x1 <= x2 <= w and 0 <= y1 <= y2 <= h, (n, k, (x1, y1, x2, y2), (w, h))
            assert at == L["patch_base"] + (n * Gmax + k) * L["cap"] and (y2 - y1) * (x2 - x1) * 3 <= L["cap"], (n, k)
            assert at + L["cap"] <= L["words"]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
WANTED = (["crop_taken", "mode_none", "crop_drops_tube", "erase_2plus", "aspect_continue", "erase_reject", ("mirror", True), ("mirror", False),
           ("contrast_first", True), ("contrast_first", False)] +
          [(n, v) for n in ("brightness", "contrast", "saturation", "hue", "perm") for v in (True, False)])
_GRID = {}


def grid():
    """the 64 pairs x 6 switch combinations, restated once; asserts its own coverage -> {(switches, seed, offset): restated}"""
    if not _GRID:
        seen = set()
        gt, cnt = make_gt()
        for sw in COMBOS:
            for seed, offset in PAIRS:
                _RESTATED[(sw, seed, offset, False)] = _GRID[(sw, seed, offset)] = restate(DIMS, gt, cnt, sw, seed, offset, seen=seen)
        missing = [w for w in WANTED if w not in seen]
        assert not missing, ("the cases never took these branches", missing)
        assert "crop_outside" not in seen
    return _GRID


def qualifies(want):
    return not any(r["crop_cap"] or r["erase_cap"] for r in want[4])


def case_words_are_the_librarys(bk):
    """philox_words, which the restatement draws from, is step_rng_words on the blocks the rule addresses (every phase, clips 0 and 2, the
    noise offset)"""
    for seed, offset in (PAIRS[0], PAIRS[21], PAIRS[63]):
        for off in (offset, offset + 1):
            st = _state(bk, seed, off)
            for first in (0, 1 << 16 | 3200, 2 << 20 | 2 << 16, 2 << 20 | 3 << 16 | 4 * 64 * 3, (2 * GMAX + 1) << 20):
                out = bk.dev(np.zeros(4 * 64, np.int32))
                assert bk.lib.step_rng_words(st.ptr, first, 64, out.ptr, bk.stream) == 0
                assert np.array_equal(out.get().view(np.uint32).reshape(64, 4).astype(u64), philox_words(seed, off, first, 64))


def case_equals_restatement(bk, part):
    """64 (seed, offset) pairs x {all on, each switch alone, none}: block, patches, gt_out, gt_count_out bit for bit; the offset moves by 2.
    part 0..23: one switch combination and 16 of the pairs (the host interpreter takes a quarter of a second per call)"""
    gt, cnt = make_gt()
    call = Call(bk, DIMS, gt, cnt)
    for (sw, seed, offset), want in list(grid().items())[16 * part:16 * part + 16]:
        call.fresh()
        st = _state(bk, seed, offset)
        assert call.run(st, sw) == 0
        same_outputs(call, want, (sw, seed, offset))
        assert _read_state(st) == (seed, (offset + 2) & 0xFFFFFFFFFFFFFFFF)
        assert not any(r["dropped"] for r in want[4])


def case_other_parameters(bk):
    """the noise ranges of scale 0 and 1, another network resolution, a block sized for larger frames than the batch holds, a single clip
    and an empty batch (which still counts as a call)"""
    gt, cnt = make_gt()
    seed, offset = PAIRS[9]
    for scale, Wn, Hn, max_hw in ((0, WN, HN, MAX_HW), (1, 400, 320, MAX_HW), (2, 7, 9, 3 * MAX_HW + 1)):
        call = Call(bk, DIMS, gt, cnt, max_hw=max_hw)
        st = _state(bk, seed, offset)
        assert call.run(st, ALL, scale=scale, Wn=Wn, Hn=Hn) == 0
        same_outputs(call, restate(DIMS, gt, cnt, ALL, seed, offset, scale, Wn, Hn, max_hw), (scale, Wn, Hn, max_hw))
    call = Call(bk, DIMS[1:2], gt[1:2], cnt[1:2])
    st = _state(bk, seed, offset)
    assert call.run(st, ALL) == 0
    same_outputs(call, restate(DIMS[1:2], gt[1:2], cnt[1:2], ALL, seed, offset), "one clip")
    st = _state(bk, seed, offset)
    assert call.run(st, ALL, N=0, src=None, dims=None, gt=None, cnt=None, block=None, gt_out=None, cnt_out=None) == 0
    assert _read_state(st) == (seed, offset + 2)


def case_conforms_to_host_rule():
    """TubeAugmentation.plan, fed the draws the restatement consumed, returns the restated AugPlan and tubes bit for bit -- over the
    all-on cases that hit neither cap, which must be at least 48 of the 64"""
    gt, cnt = make_gt()
    ok = 0
    for seed, offset in PAIRS:
        want = grid()[(ALL, seed, offset)]
        if not qualifies(want):
            continue
        ok += 1
        for sw in COMBOS:
            recs = grid()[(sw, seed, offset)][4]
            if sw != ALL and any(r["crop_cap"] or r["erase_cap"] for r in recs):
                continue
            aug = TubeAugmentation((WN, HN), MEAN, STDS, bool(sw & FLIP), bool(sw & CROP), bool(sw & PHOTO), bool(sw & ERASE), scale=SCALE)
            for n, rec in enumerate(recs):
                G = int(cnt[n])
                if G == 0 and (sw & CROP) and rec["mode_first"] != 0:
                    try:                                                       # the host form has no answer here: numpy's min() of no overlaps
                        host_plan(aug, DIMS[n], gt[n, :G], rec)
                    except ValueError:
                        continue
                    raise AssertionError("the host rule evaluated a crop trial without tubes")
                plan, tubes = host_plan(aug, DIMS[n], gt[n, :G], rec)
                assert AC.same_plan(plan, plan_of(rec)), (sw, seed, offset, n)
                assert AC.same_array(tubes, rec["tubes_pct"]), (sw, seed, offset, n)
    assert ok >= 48, ok


def case_caps(bk):
    """a state whose crop runs through 16 rounds (the clip without tubes: no trial keeps a box) and keeps the whole frame, and one whose
    thin box is rejected by 64 get_region trials and gets no rectangle; kernel == restatement for both.

    The thin box of the erase cap is the SLIVER of make_gt (0.02 px wide), not the 3 px one: get_region accepts a trial when We =
    sqrt(Se / re) fits the box, Se / re >= 0.02 S / (10/3), and a 3 px box in a frame of at most 47 px accepts about two trials in three --
    64 rejections in a row are beyond any search.  A 0.02 px box rejects every trial, so the state only has to throw the erase coin."""
    gt, cnt = make_gt()
    seed, offset = CROP_CAP_STATE
    want = restated(ALL, seed, offset)
    assert want[4][2]["crop_cap"] and want[4][2]["crop"] == (0, 0, DIMS[2][1], DIMS[2][0])
    call = Call(bk, DIMS, gt, cnt)
    st = _state(bk, seed, offset)
    assert call.run(st, ALL) == 0
    same_outputs(call, want, "crop cap")
    gt, cnt = make_gt(sliver=True)
    seed, offset = ERASE_CAP_STATE
    want = restated(ERASE, seed, offset, sliver=True)
    r = want[4][1]
    assert r["erase_coin"] and r["erase_cap"] and len(r["rects"]) == r["K"] - 1 == 3 and not r["dropped"]
    call = Call(bk, DIMS, gt, cnt)
    st = _state(bk, seed, offset)
    assert call.run(st, ERASE) == 0
    same_outputs(call, want, "erase cap")
    assert read_block(call.block.get().view(np.int32), 3, GMAX)[1]["rects"] == [tuple(v) for v in r["rects"]]


def _frames():
    rs = np.random.RandomState(3)
    return [rs.randint(0, 256, (T, h, w, 3)).astype(np.uint8) for h, w in DIMS]


def case_pixels(bk):
    """the device-made block through step_clip_augment_u8 == augment_cases.np_apply of the plans read back from it: fp32 bit-equal,
    bf16 / fp16 the round-to-nearest-even of that"""
    gt, cnt = make_gt()
    frames = _frames()
    call = Call(bk, DIMS, gt, cnt, frames=frames)
    m, sd = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STDS)
    for seed, offset in (PAIRS[3], PAIRS[18], PAIRS[44]):
        st = _state(bk, seed, offset)
        assert call.run(st, ALL) == 0
        words = call.block.get().view(np.int32)
        block_is_safe(words, 3, GMAX, DIMS, call.L)
        plans = [plan_of(r) for r in read_block(words, 3, GMAX)]
        want = np.stack([AC.nchw(AC.np_apply(fr, p, (WN, HN), SCALE, MEAN, STDS), True) for fr, p in zip(frames, plans)])
        for dt, bits in ((AC.F32, want), (AC.BF16, AC.to_bf16_bits(want)), (AC.F16, want.astype(np.float16).view(np.uint16))):
            out = bk.dev(np.zeros((3, T, 3, HN, WN), np.float32 if dt == AC.F32 else np.uint16))
            assert bk.lib.step_clip_augment_u8(call.block.ptr, 3, T, HN, WN, SCALE, m, sd, 1, dt, out.ptr, bk.stream) == 0
            assert np.array_equal(out.get().view(bits.dtype), bits), (seed, offset, dt)


SAFETY_SEED = 77


def case_safety_restated():
    """1000 offsets on the restatement: every block is safe and no rectangle was dropped for its size or place"""
    gt, cnt = make_gt()
    L = layout(3, GMAX, MAX_HW)
    for offset in range(1000):
        want = restated(ALL, SAFETY_SEED, offset)
        block_is_safe(want[0], 3, GMAX, DIMS, L)
        assert not any(r["dropped"] for r in want[4]), offset


def case_safety_kernel(bk, part):
    """64 of those offsets on the kernel, 16 per part: safe blocks, equal to the restatement"""
    gt, cnt = make_gt()
    call = Call(bk, DIMS, gt, cnt)
    for offset in range(0, 1000, 15)[16 * part:16 * part + 16]:
        st = _state(bk, SAFETY_SEED, offset)
        assert call.run(st, ALL) == 0
        block_is_safe(call.block.get().view(np.int32), 3, GMAX, DIMS, call.L)
        same_outputs(call, restated(ALL, SAFETY_SEED, offset), offset)


COIN_SEED = 4242


def case_coins(bk):
    """over 512 offsets the mirror and the erase coin of clip 0 each come up in 0.5 +- 0.1 (4.5 binomial standard deviations at n = 512).
    Counted on the restatement over all 512; the kernel's block -- the mirror flag; a rectangle, which clip 0's boxes get whenever the coin
    says erase (asserted of the restatement) -- must agree at every offset on the GPU and at every 8th on the host interpreter, which
    spends 30 ms on a call whatever its size."""
    gt, cnt = make_gt()
    call = Call(bk, DIMS[:1], gt[:1, :2], cnt[:1])
    mirror = erase = 0
    for offset in range(512):
        r = restate_clip(0, DIMS[0], gt[0, :2], int(cnt[0]), FLIP | ERASE, WN, HN, call.L["cap"], COIN_SEED, offset)
        assert r["erase_coin"] == (len(r["rects"]) > 0)
        mirror += int(r["mirror"])
        erase += int(r["erase_coin"])
        if bk.name == "emul" and offset % 8:
            continue
        st = _state(bk, COIN_SEED, offset)
        assert call.run(st, FLIP | ERASE) == 0
        c = call.block.get().view(np.int32)[:16]
        assert (bool(c[8] & 1), int(c[14])) == (r["mirror"], len(r["rects"])), offset
    assert abs(mirror / 512 - 0.5) <= 0.1 and abs(erase / 512 - 0.5) <= 0.1, (mirror, erase)


def case_bad_arguments(bk):
    """every error of the header is returned, with nothing written and the offset where it was"""
    gt, cnt = make_gt()
    call = Call(bk, DIMS, gt, cnt)
    st = _state(bk, 5, 9)
    big = Call(bk, ((4, 4),), np.zeros((1, 65, 1, 4), f32), [0])
    for want, o in ((E_SHAPE, dict(N=-1)), (E_SHAPE, dict(Gmax=-1)), (E_SHAPE, dict(F=0)), (E_SHAPE, dict(NC=-1)), (E_SHAPE, dict(Wn=0)),
                    (E_SHAPE, dict(Hn=0)), (E_SHAPE, dict(max_hw=0)), (E_SHAPE, dict(scale=3)), (E_SHAPE, dict(scale=-1)),
                    (E_SHAPE, dict(switches=16)), (E_UNSUPPORTED, dict(max_hw=1 << 40)), (E_NULL, dict(rng=None)), (E_NULL, dict(block=None)),
                    (E_NULL, dict(src=None)), (E_NULL, dict(dims=None)), (E_NULL, dict(gt=None)), (E_NULL, dict(cnt=None)),
                    (E_NULL, dict(gt_out=None)), (E_NULL, dict(cnt_out=None)), (E_ALIGN, dict(block=_addr(call.block.ptr) + 4)),
                    (E_ALIGN, dict(rng=_addr(st.ptr) + 4))):
        assert call.run(st, **o) == want, (want, o)
        assert call.untouched() and _read_state(st) == (5, 9), o
    assert big.run(st, ALL) == E_UNSUPPORTED and big.untouched() and _read_state(st) == (5, 9)              # Gmax 65
    assert bk.lib.step_augment_plan_bytes(-1, 4, 100, None) == 0 and bk.lib.step_augment_plan_bytes(1, 4, 0, None) == 0


KERNEL_CASES = (["case_words_are_the_librarys"] + ["case_equals_restatement:%d" % k for k in range(24)] +
                ["case_other_parameters", "case_caps", "case_pixels"] + ["case_safety_kernel:%d" % k for k in range(4)] + ["case_coins", "case_bad_arguments"])


def run_kernel_case(name, bk):
    fn, _, part = name.partition(":")
    return globals()[fn](bk, int(part)) if part else globals()[fn](bk)
HOST_CASES = ["case_conforms_to_host_rule", "case_safety_restated"]

# Found by CPU searches with the restatement alone (find_cap_states below), committed as constants.
CROP_CAP_STATE = (0, 0)
ERASE_CAP_STATE = (0, 0)


def find_cap_states(limit=4000):
    """the searches behind the two constants: the first (seed, 0) whose clip 2 runs through 16 crop rounds / whose clip 1 throws the erase coin"""
    gt, cnt = make_gt()
    crop = next((s, 0) for s in range(limit) if restate_clip(2, DIMS[2], gt[2], 0, CROP, WN, HN, 1 << 20, s, 0)["crop_cap"])
    gts, _ = make_gt(sliver=True)
    erase = next((s, 0) for s in range(limit) if restate_clip(1, DIMS[1], gts[1], 4, ERASE, WN, HN, 1 << 20, s, 0)["erase_coin"])
    return crop, erase


# ---- the module ----------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    import torch

    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16) if t.dtype in (torch.bfloat16, torch.float16) else t.detach().cpu().numpy()


def module_inputs(device):
    import torch

    gt, cnt = make_gt()
    return gt, cnt, [torch.from_numpy(f).to(device) for f in _frames()], torch.from_numpy(gt).to(device), torch.from_numpy(cnt).to(device)


def check_apply(aug, res, seed, offset, frames, gt, cnt, rgb=True):
    """one apply() against the restatement at (seed, offset): block, ground truths, and the pixels np_apply makes of the restated plans"""
    out, gt_out, cnt_out = res
    want = restate(DIMS, gt, cnt, aug.switches, seed, offset)
    words = aug.last_block().cpu().numpy().view(np.int32).copy()
    words[:16 * 3].reshape(3, 16)[:, :2] = 0
    head = layout(3, GMAX, MAX_HW)["patch_base"]
    assert np.array_equal(words[:head], want[0][:head])
    for a, b in want[1]:
        assert np.array_equal(words[a:b], want[0][a:b])
    assert np.array_equal(gt_out.cpu().numpy().view(np.int32), want[2].view(np.int32)) and np.array_equal(cnt_out.cpu().numpy(), want[3])
    pix = np.stack([AC.nchw(AC.np_apply(fr, plan_of(r), (WN, HN), SCALE, MEAN, STDS), rgb) for fr, r in zip(frames, want[4])])
    import torch
    bits = {torch.float32: pix, torch.bfloat16: AC.to_bf16_bits(pix), torch.float16: pix.astype(np.float16).view(np.uint16)}[out.dtype]
    assert np.array_equal(_bits(out), bits)


def module_apply_equals_restatement(device):
    """DeviceTubeAugmentation.apply on a list of clips of three sizes: three calls draw at offsets o, o + 2, o + 4; the default output is
    bf16 with the rgb swap; out= / gt_out= / gt_count_out= are filled in place (out's dtype wins); last_block() is the block"""
    import torch

    import step_amd
    gt, cnt, clips, d_gt, d_cnt = module_inputs(device)
    rng = step_amd.DeviceRNG(device, seed=21)
    rng.set_state((21, 5))
    aug = step_amd.DeviceTubeAugmentation((WN, HN), MEAN, STDS, True, True, True, True, scale=SCALE, rng=rng)
    res = aug.apply(clips, d_gt, d_cnt)
    assert res[0].dtype == torch.bfloat16 and rng.get_state() == (21, 7)
    check_apply(aug, res, 21, 5, _frames(), gt, cnt)
    block = aug.last_block()
    res = aug.apply(clips, d_gt, d_cnt, dtype=torch.float32, rgb=False)
    assert aug.last_block() is block and rng.get_state() == (21, 9)
    check_apply(aug, res, 21, 7, _frames(), gt, cnt, rgb=False)
    out = torch.full((3, T, 3, HN, WN), 7.0, dtype=torch.float16, device=device)
    g_out, c_out = torch.full_like(d_gt, 7.0), torch.full_like(d_cnt, 7)
    res = aug.apply(clips, d_gt, d_cnt, out=out, gt_out=g_out, gt_count_out=c_out, dtype=torch.float32)
    assert res[0] is out and res[1] is g_out and res[2] is c_out
    check_apply(aug, res, 21, 9, _frames(), gt, cnt)
    only = step_amd.DeviceTubeAugmentation((WN, HN), MEAN, STDS, do_crop=True, scale=SCALE, rng=rng)         # one switch; one [N,T,H,W,3] tensor
    same = torch.from_numpy(np.stack([_frames()[0]] * 2)).to(device)
    res = only.apply(same, d_gt[:2].contiguous(), d_cnt[:2].contiguous(), dtype=torch.float32)
    want = restate(DIMS[:1] * 2, gt[:2], cnt[:2], CROP, 21, 11)
    assert np.array_equal(res[1].cpu().numpy().view(np.int32), want[2].view(np.int32)) and rng.get_state() == (21, 13)


def module_refuses_bad_input(device):
    import pytest
    import torch

    import step_amd
    gt, cnt, clips, d_gt, d_cnt = module_inputs(device)
    rng = step_amd.DeviceRNG(device, seed=1)
    aug = step_amd.DeviceTubeAugmentation((WN, HN), rng=rng, scale=SCALE)
    with pytest.raises(RuntimeError):
        step_amd.DeviceTubeAugmentation((WN, HN)).apply(clips, d_gt, d_cnt)                    # no generator
    with pytest.raises(RuntimeError):
        aug.last_block()
    for bad in (lambda: aug.apply([c.float() for c in clips], d_gt, d_cnt), lambda: aug.apply(clips[:2], d_gt, d_cnt),
                lambda: aug.apply(clips, d_gt.double(), d_cnt), lambda: aug.apply(clips, d_gt, d_cnt.long()),
                lambda: aug.apply(clips, d_gt, d_cnt, out=torch.zeros((3, T, 3, HN, WN + 1), device=device)),
                lambda: aug.apply(clips, d_gt, d_cnt, gt_out=torch.zeros((3, GMAX, F, 4), device=device)),
                lambda: aug.apply(clips, d_gt, d_cnt, gt_count_out=torch.zeros(3, device=device))):
        with pytest.raises(RuntimeError):
            bad()
    assert rng.get_state() == (1, 0)
    with pytest.raises(ValueError):
        step_amd.DeviceTubeAugmentation((WN, HN), rng=rng, scale=3)


def module_selector_follows_changing_ground_truths(device):
    """DeviceSelector(dynamic_gt=True) gathers the middle-frame boxes on every select(): after the ground truths were rewritten in place
    WITHOUT a version bump (what a kernel writing through a raw pointer does), its step-2 selection equals that of a fresh selector on the
    new boxes, while the default form -- unchanged: it hands back its cached tensor -- still holds the old ones."""
    import torch

    import step_amd
    from step_amd.selection import DeviceSelector
    from tests import select_cases as SC

    rs = np.random.RandomState(21)
    tubes, gts = [9, 4, 12], [2, 1, 3]
    a = SC.cfg()
    inp, _, _, flat, hist = SC._module_inputs(rs, tubes, gts, a.num_classes, near=0.7, spread=12)
    gt, gt_count, init_flat, clip_start, pads, dhist = SC._device_args(device, inp, flat, hist, a)
    rng = step_amd.DeviceRNG(device, seed=41)
    cached, live = DeviceSelector(a, 3, 15, device, rng), DeviceSelector(a, 3, 15, device, rng, dynamic_gt=True)
    assert not cached.dynamic_gt

    def run(sel):
        rng.set_state((41, 7))
        return [SC.np_(t).copy() for t in sel.select(2, dhist[0], gt, gt_count, init_flat, clip_start, pads[2], max_tubes=12)]

    first = run(cached)
    assert all(np.array_equal(x, y) for x, y in zip(first, run(live)))
    held = cached._gt_mid_boxes(gt, 1)
    assert cached._gt_mid_boxes(gt, 1) is held                                  # the default: one gather per tensor version
    moved = gt.clone()
    moved[:, :, :, :4] = moved[:, :, :, :4].flip(1)                             # every clip's boxes change places (labels stay)
    moved[0, :, :, 0:4:2] += 37.0
    version = gt._version
    gt.data.copy_(moved)                                                        # (.data has a version counter of its own)
    assert gt._version == version and cached._gt_mid_boxes(gt, 1) is held and not torch.equal(held, gt[:, :, 1, :4])
    want = run(DeviceSelector(a, 3, 15, device, rng))
    got = run(live)
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert not all(np.array_equal(x, y) for x, y in zip(got, first))


MODULE_CASES = ["module_apply_equals_restatement", "module_refuses_bad_input", "module_selector_follows_changing_ground_truths"]
