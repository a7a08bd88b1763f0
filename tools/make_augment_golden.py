#!/usr/bin/env python
"""tools/make_augment_golden.py -- writes tests/golden/augment_golden.npz: what the reference's loader transform
(data/augmentations.py: TubeAugmentation :540-586, BaseTransform :601-615) computes on seeded uint8 frames, tubes and proposals.

Method: the reference's `data.augmentations` is imported from where the reference lies at generation time and its two classes are called
as they stand.  Two modules it imports do not exist here and are replaced by stand-ins in `sys.modules` BEFORE the import:
  * `cv2`: `resize` (bilinear, float32), `cvtColor` with COLOR_BGR2HSV / COLOR_HSV2BGR -- written below from OpenCV's float32 formulas
    (the same ones include/step_amd.h and DESIGN.md 3.10 state); parity with a real OpenCV build is NOT established by this file, see
    --check-cv2;
  * `torchvision`: an empty module with a `transforms` attribute (imported by the reference, never used by the two classes).
numpy 2 refuses the ragged tuple RandomSampleCrop hands to `random.choice`: the instance's `sample_options` is re-held as a 1-D object
ndarray of the same seven entries (the draw is the same randint(7)).  No reference code is copied.

Observed, not computed: every transform instance of the pipeline is wrapped by a recorder (Compose only calls them), and
numpy.random's `randint` / `uniform` / `choice` are wrapped for the duration of the call, so the crop rectangle (the offset of the view the
crop returns), the mirror coin, the erase rectangles (get_region's return values) and patches, and the photometric draws are read off
the reference's own run.  After the call one more number is drawn from the stream (the sentinel) so a test can check that a plan leaves
the RNG where the reference leaves it.

The generator asserts, and prints counts for, the coverage of every branch (see COVERAGE).  Needs the reference tree; not run by the
tests, which read only the .npz.

    python tools/make_augment_golden.py [--check-cv2]
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import OUT, REF  # noqa: E402

F32 = np.float32
EPS = F32(1.1920928955078125e-7)        # FLT_EPSILON


# ---- the stand-in for cv2 -----------------------------------------------------------------------------------------------------------
def _coords(dst, src):
    """cv2.resize's bilinear source coordinates for float32: first tap, second tap, weight of the second tap."""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (float(src) / dst) - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F32)
    low, high = s < 0, s >= src - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = src - 1, 0
    return s, np.minimum(s + 1, src - 1), f.astype(F32)


def resize(img, dsize):
    """bilinear, float32: horizontal pass on the two rows, then the vertical one; equal sizes copy."""
    w, h = dsize
    assert img.dtype == F32 and img.ndim == 3
    if (img.shape[1], img.shape[0]) == (w, h):
        return img.copy()
    x0, x1, fx = _coords(w, img.shape[1])
    y0, y1, fy = _coords(h, img.shape[0])
    fx, fy = fx[None, :, None], fy[:, None, None]
    one = F32(1)
    top = img[y0][:, x0] * (one - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (one - fx) + img[y1][:, x1] * fx
    return (top * (one - fy) + bot * fy).astype(F32)


COLOR_BGR2HSV, COLOR_HSV2BGR = 40, 54


def bgr2hsv(img):
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = diff / (np.abs(v) + EPS)
    d = (60. / (diff + EPS).astype(np.float64)).astype(F32)
    h = np.where(v == r, (g - b) * d, np.where(v == g, (b - r) * d + F32(120), (r - g) * d + F32(240))).astype(F32)
    h = np.where(h < 0, h + F32(360), h)
    return np.stack([h, s, v], -1).astype(F32)


def hsv2bgr(img):
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    one = F32(1)
    h = h * (F32(6) / F32(360))
    while (h < 0).any():
        h = np.where(h < 0, h + F32(6), h)
    while (h >= 6).any():
        h = np.where(h >= 6, h - F32(6), h)
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(F32)
    out_of_range = (sector < 0) | (sector >= 6)
    sector = np.where(out_of_range, 0, sector)
    h = np.where(out_of_range, F32(0), h)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], -1)
    table = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    bgr = np.take_along_axis(tab, table[sector], -1)
    return np.where((s == 0)[..., None], v[..., None], bgr).astype(F32)


def cvtColor(img, code):
    assert img.dtype == F32 and img.shape[-1] == 3
    with np.errstate(all="ignore"):
        return bgr2hsv(img) if code == COLOR_BGR2HSV else hsv2bgr(img)


def install_stand_ins():
    cv2 = types.ModuleType("cv2")
    cv2.resize, cv2.cvtColor, cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = resize, cvtColor, COLOR_BGR2HSV, COLOR_HSV2BGR
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules["cv2"], sys.modules["torchvision"], sys.modules["torchvision.transforms"] = cv2, tv, tv.transforms


# ---- observing one call of the reference ----------------------------------------------------------------------------------------------
class Recorder:
    """Stands where a transform instance stood in a Compose list: calls it and keeps what went in and what came out."""

    def __init__(self, inner, log, calls):
        self.inner, self.log, self.calls = inner, log, calls

    def get_name(self):
        return self.inner.get_name()

    def __call__(self, images, tubes=None, proposals=None):
        before = images.copy()
        start = len(self.log)
        out = self.inner(images, tubes, proposals)
        self.calls.append(dict(inner=self.inner, kind=type(self.inner).__name__, before=before, images_in=images, out=out[0],
                               draws=self.log[start:]))
        return out


def observe(A, aug, frames, tubes, proposals, seed):
    """One seeded call of the reference's transform with every stage and every draw recorded."""
    log, calls, regions = [], [], []
    steps = aug.augment.transforms
    saved_steps = list(steps)
    saved_inner = []
    for k, t in enumerate(saved_steps):
        name = type(t).__name__
        if name == "RandomSampleCrop":
            held = np.empty(len(t.sample_options), dtype=object)                # the 1-D object hold of the 7 entries
            for j, mode in enumerate(t.sample_options):
                held[j] = mode
            t.sample_options = held
        if name == "RandomErase":
            bound = t.get_region
            t.get_region = lambda box, bound=bound: regions.append(bound(box)) or regions[-1]
            saved_inner.append((t, "get_region"))
        if name == "PhotometricDistort":
            saved_inner.append((t, list(t.pd), t.rand_brightness, t.rand_light_noise))
            t.pd = [Recorder(x, log, calls) for x in t.pd]
            t.rand_brightness, t.rand_light_noise = Recorder(t.rand_brightness, log, calls), Recorder(t.rand_light_noise, log, calls)
        steps[k] = Recorder(t, log, calls)
    real = {n: getattr(np.random, n) for n in ("randint", "uniform", "choice")}

    def logged(n):
        def f(*a, **kw):
            v = real[n](*a, **kw)
            log.append((n, a, v))
            return v
        return f
    try:
        for n in real:
            setattr(np.random, n, logged(n))
        np.random.seed(seed)
        out = aug(frames.copy(), None if tubes is None else tubes.copy(), None if proposals is None else proposals.copy())
    finally:
        for n, fn in real.items():
            setattr(np.random, n, fn)
        steps[:] = saved_steps
        for item in saved_inner:
            if item[1] == "get_region":
                del item[0].get_region
            else:
                item[0].pd, item[0].rand_brightness, item[0].rand_light_noise = item[1], item[2], item[3]
    sentinel = np.random.random_sample()
    return out, calls, regions, sentinel


def read_plan(calls, regions, frames):
    """The plan quantities, read off the recorded run."""
    T, H, W, _ = frames.shape
    q = dict(crop=[0, 0, W, H], mirror=0, photo=np.zeros(6, np.int32), params=np.zeros(4, F32), perm=[0, 1, 2], rects=np.zeros((0, 4), np.int64),
             patches=np.zeros(0, F32), hue_wrap=[0, 0], grey=0, black=0, dropped=0)
    seen_contrast = 0
    for c in calls:
        kind, draws = c["kind"], c["draws"]
        coin = bool(draws[0][2]) if draws and draws[0][0] == "randint" else False
        if kind == "PhotometricDistort":
            q["photo"][0] = 1
        elif kind == "RandomBrightness" and coin:
            q["photo"][1], q["params"][0] = 1, F32(draws[1][2])
        elif kind == "RandomContrast":
            if coin:
                q["photo"][2], q["params"][1] = 1, F32(draws[1][2])
        elif kind == "ConvertColor" and c["inner"].transform == "HSV":
            q["photo"][3] = seen_contrast                                   # contrast first: a RandomContrast ran before the HSV trip
            px = c["before"]
            q["grey"] += int((px.max(-1) == px.min(-1)).sum())
            q["black"] += int((px.max(-1) == 0).sum())
        elif kind == "RandomSaturation" and coin:
            q["photo"][4], q["params"][2] = 1, F32(draws[1][2])
        elif kind == "RandomHue" and coin:
            q["photo"][5], q["params"][3] = 1, F32(draws[1][2])
            t = c["before"][..., 0] + q["params"][3]
            q["hue_wrap"] = [int((t > 360).sum()), int((t < 0).sum())]
        elif kind == "RandomLightingNoise" and coin:
            q["perm"] = list(c["inner"].perms[int(draws[1][2])])
        elif kind == "RandomSampleCrop":
            src, dst = c["images_in"], c["out"]
            if dst is not src:
                off = dst.__array_interface__["data"][0] - src.__array_interface__["data"][0]
                y = off // src.strides[1]
                x = (off - y * src.strides[1]) // src.strides[2]
                assert np.shares_memory(src, dst) and src.strides[1] >= src.strides[2] * src.shape[2] and y * src.strides[1] + x * src.strides[2] == off
                q["crop"] = [int(x), int(y), int(dst.shape[2]), int(dst.shape[1])]
        elif kind == "RandomMirror":
            q["mirror"] = int(coin)
        elif kind == "RandomErase" and coin:
            q["rects"] = np.array(regions, np.int64).reshape(-1, 4)
            sized = [d for d in draws if d[0] == "uniform" and len(d[1]) == 3]
            assert len(sized) == len(regions)
            q["patches"] = np.concatenate([np.zeros(0, F32)] + [d[2].astype(F32).reshape(-1) for d in sized])
        if kind == "RandomContrast":
            seen_contrast = 1
    # contrast first is decided by the ORDER of the recorded calls: the first RandomContrast call precedes the HSV conversion
    kinds = [c["kind"] for c in calls]
    if "ConvertColor" in kinds:
        q["photo"][3] = int("RandomContrast" in kinds[:kinds.index("ConvertColor")])
    return q


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
MEANS, STDS = (0.1, -0.2, 0.3), (0.9, 1.1, 1.3)


def make_inputs(rs, T, H, W, n_tubes, n_props, overlap):
    frames = rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8)
    frames[:, 1::7, 2::5] = frames[:, 1::7, 2::5, :1]                      # grey pixels (diff == 0)
    frames[:, 3::11, 1::9] = 0                                              # black pixels (v == 0)
    frames[:, ::13, ::6] = 255
    def boxes(n, T_):
        if overlap:
            c = np.array([0.5, 0.5]) + rs.uniform(-0.08, 0.08, (n, 2))
            half = rs.uniform(0.25, 0.4, (n, 2))
        else:
            c = rs.uniform(0.15, 0.85, (n, 2))
            half = rs.uniform(0.08, 0.15, (n, 2))
        b = np.concatenate([np.clip(c - half, 0, 1), np.clip(c + half, 0, 1)], 1)
        return np.tile(b[:, None, :], (1, T_, 1))
    tubes = boxes(n_tubes, T).astype(F32)
    tubes = np.concatenate([tubes, rs.randint(0, 2, (n_tubes, T, 3)).astype(F32)], 2)        # label columns ride along
    props = boxes(n_props, T).astype(np.float64) if n_props else None
    return frames, tubes, props


def overlapping(r):
    for i in range(len(r)):
        for j in range(i + 1, len(r)):
            if min(r[i][2], r[j][2]) > max(r[i][0], r[j][0]) and min(r[i][3], r[j][3]) > max(r[i][1], r[j][1]):
                return True
    return False


ALL = dict(do_flip=True, do_crop=True, do_photometric=True, do_erase=True)
# name: (kind, (Hs, Ws), (Wo, Ho), scale, mean, stds, switches, tubes, proposals, overlapping tubes, predicate on the observed plan q / tubes)
CASES = [
    ("A", "tube", (48, 64), (32, 32), 2, (0, 0, 0), (1, 1, 1), ALL, 2, 3, True,
     lambda q: q["crop"][2:] != [64, 48] and q["mirror"] and len(q["rects"]) >= 2 and overlapping(q["rects"]) and q["photo"][3] and q["photo"][2]),
    ("B", "tube", (36, 48), (40, 24), 2, (0, 0, 0), (1, 1, 1), ALL, 2, 0, False,
     lambda q: q["crop"] == [0, 0, 48, 36] and not q["mirror"] and not q["photo"][3] and q["photo"][5] and q["hue_wrap"][0]),
    ("C", "tube", (48, 64), (32, 32), 2, MEANS, STDS, ALL, 3, 2, False,
     lambda q: q["dropped"] > 0 and q["perm"] != [0, 1, 2] and q["photo"][1] and q["photo"][4]),
    ("D", "tube", (40, 56), (32, 32), 1, MEANS, STDS, ALL, 2, 2, True,
     lambda q: not q["photo"][1] and not q["photo"][2] and q["photo"][4] and len(q["rects"]) >= 1),
    ("E", "tube", (40, 56), (32, 32), 0, MEANS, STDS, ALL, 2, 0, True,
     lambda q: len(q["rects"]) >= 1 and not q["photo"][4] and not q["photo"][5] and q["photo"][2]),
    ("F", "tube", (32, 32), (32, 32), 2, (0, 0, 0), (1, 1, 1), dict(do_photometric=True), 1, 0, False,
     lambda q: q["photo"][5] and q["hue_wrap"][1] and q["photo"][2] and not q["photo"][3]),
    ("G", "tube", (24, 32), (40, 40), 2, (0, 0, 0), (1, 1, 1), dict(do_flip=True, do_crop=True, do_erase=True), 2, 2, True,
     lambda q: q["crop"][2:] != [32, 24] and len(q["rects"]) >= 2),
    ("H", "tube", (64, 80), (40, 32), 1, MEANS, STDS, dict(do_flip=True), 2, 1, False, lambda q: q["mirror"]),
    ("I", "base", (48, 64), (32, 32), 1, MEANS, STDS, {}, 2, 1, False, None),
    ("J", "base", (32, 40), (40, 32), 2, (0, 0, 0), (1, 1, 1), {}, 0, 0, False, None),
    ("K", "base", (20, 28), (40, 40), 0, MEANS, STDS, {}, 0, 0, False, None),
    ("L", "tube", (36, 48), (32, 32), 2, (0, 0, 0), (1, 1, 1), {}, 2, 0, False, None),
]
T_FRAMES = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-cv2", action="store_true",
                    help="where a real cv2 imports: compare the stand-in's resize / cvtColor with it on the cases' frames and print the largest difference")
    a = ap.parse_args()
    if a.check_cv2:
        return check_cv2()
    install_stand_ins()
    sys.path.insert(0, REF)
    import data.augmentations as A                                          # reference

    g, cov = {}, {}

    def count(name, on):
        cov[name] = cov.get(name, 0) + int(bool(on))

    for name, kind, (Hs, Ws), size, scale, mean, stds, sw, n_t, n_p, ov, want in CASES:
        for seed in range(1000 * (ord(name) - 64), 1000 * (ord(name) - 64) + 4000):
            rs = np.random.RandomState(seed)
            frames, tubes, props = make_inputs(rs, T_FRAMES, Hs, Ws, max(n_t, 1), n_p, ov)
            if kind == "tube":
                aug = A.TubeAugmentation(size, mean, stds, scale=scale, **sw)
            else:
                aug = A.BaseTransform(size, mean, stds, scale=scale)
                if n_t == 0:
                    tubes = None
            (out, tubes_out, props_out), calls, regions, sentinel = observe(A, aug, frames, tubes, props, seed)
            q = read_plan(calls, regions, frames)
            q["dropped"] = 0 if tubes is None else len(tubes) - len(tubes_out)
            if want is None or want(q):
                break
        else:
            raise SystemExit("case %s: no seed satisfies its predicate" % name)
        assert out.dtype == F32 and out.shape == (T_FRAMES, size[1], size[0], 3)
        k = "%s_" % name
        g[k + "seed"], g[k + "kind"], g[k + "size"], g[k + "scale"] = np.int64(seed), np.int32(kind == "base"), np.array(size, np.int32), np.int32(scale)
        g[k + "mean"], g[k + "stds"] = np.array(mean, np.float64), np.array(stds, np.float64)
        g[k + "switches"] = np.array([sw.get(n, False) for n in ("do_flip", "do_crop", "do_photometric", "do_erase")], np.int32)
        g[k + "frames"] = frames
        if tubes is not None:
            g[k + "tubes_in"], g[k + "tubes_out"] = tubes, tubes_out
        if props is not None:
            g[k + "props_in"], g[k + "props_out"] = props, props_out
        g[k + "out"], g[k + "sentinel"] = out, np.float64(sentinel)
        g[k + "crop"], g[k + "mirror"], g[k + "photo"], g[k + "params"] = np.array(q["crop"], np.int32), np.int32(q["mirror"]), q["photo"], q["params"]
        g[k + "perm"], g[k + "rects"], g[k + "patches"] = np.array(q["perm"], np.int32), q["rects"].astype(np.int32), q["patches"]
        cw, ch = q["crop"][2:]
        print("case %s seed %d: crop %s mirror %d photo %s params %s perm %s rects %s hue wraps %s tubes %s -> %s" % (
            name, seed, q["crop"], q["mirror"], q["photo"].tolist(), q["params"].tolist(), q["perm"], q["rects"].tolist(), q["hue_wrap"],
            None if tubes is None else tubes.shape, None if tubes_out is None else tubes_out.shape))
        tube = kind == "tube"
        count("crop taken", tube and sw.get("do_crop") and [cw, ch] != [Ws, Hs])
        count("crop mode None", tube and sw.get("do_crop") and [cw, ch] == [Ws, Hs])
        count("crop drops a tube", q["dropped"] > 0)
        count("mirror on", q["mirror"])
        count("mirror off", tube and sw.get("do_flip") and not q["mirror"])
        count("erase with >= 2 rectangles", len(q["rects"]) >= 2)
        count("erase rectangles overlap", overlapping(q["rects"]))
        count("contrast first", q["photo"][0] and q["photo"][3])
        count("contrast last", q["photo"][0] and not q["photo"][3])
        for j, n in ((1, "brightness"), (2, "contrast"), (4, "saturation"), (5, "hue")):
            count(n + " on", q["photo"][0] and q["photo"][j])
            count(n + " off", q["photo"][0] and not q["photo"][j])
        count("hue wrap > 360", q["hue_wrap"][0])
        count("hue wrap < 0", q["hue_wrap"][1])
        count("channel permutation", q["perm"] != [0, 1, 2])
        count("grey pixels at the HSV conversion", q["grey"])
        count("black pixels at the HSV conversion", q["black"])
        count("up-scaling", size[0] > cw and size[1] > ch)
        count("down-scaling", size[0] < cw and size[1] < ch)
        count("exact 2x down-scaling", 2 * size[0] == cw and 2 * size[1] == ch)
        count("identity resize", size[0] == cw and size[1] == ch)
        for s in (0, 1, 2):
            count("scale %d" % s, scale == s)
        count("non-trivial mean and std", mean != (0, 0, 0))
        count("proposals present", props is not None)
        count("proposals absent", props is None)
        count("BaseTransform", kind == "base")
        count("non-square output", size[0] != size[1])
    g["cases"] = np.array([c[0] for c in CASES])
    print("COVERAGE")
    for n, v in cov.items():
        print("  %-40s %d" % (n, v))
    missing = [n for n, v in cov.items() if v == 0]
    assert not missing, "branches without a case: %s" % missing
    path = os.path.join(OUT, "augment_golden.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 833753, "larger than the largest fixture already committed"


def check_cv2():
    """Stand-in against a real OpenCV, where one imports (not available where this fixture was made)."""
    import cv2
    rs = np.random.RandomState(0)
    img = rs.uniform(-40, 300, (48, 64, 3)).astype(F32)
    worst = {}
    for size in ((32, 32), (40, 24), (64, 48), (32, 24), (100, 90)):
        worst["resize %s" % (size,)] = float(np.abs(cv2.resize(img, size) - resize(img, size)).max())
    hsv = cv2.cvtColor(img, cv2.COLOR_BGR2HSV)
    worst["BGR2HSV"] = float(np.abs(hsv - cvtColor(img, COLOR_BGR2HSV)).max())
    worst["HSV2BGR"] = float(np.abs(cv2.cvtColor(hsv, cv2.COLOR_HSV2BGR) - cvtColor(hsv, COLOR_HSV2BGR)).max())
    for n, v in worst.items():
        print("largest |cv2 - stand-in|  %-20s %.3g" % (n, v))


if __name__ == "__main__":
    main()
