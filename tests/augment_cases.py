"""Device-side clip augmentation (step_amd/augment.py, step_clip_augment_u8): the cases shared by the interpreter run
(tests/test_emul_augment.py) and the run on the real gfx950 library (tests/test_gpu_augment.py).

The fixture tests/golden/augment_golden.npz (tools/make_augment_golden.py) holds, per case, what the REFERENCE's TubeAugmentation /
BaseTransform computed on seeded uint8 frames, tubes and proposals -- the float32 [T,Ho,Wo,3] output, the returned tubes and proposals --
and the decisions observed in that run (crop, mirror, erase rectangles and patches, photometric draws, one sentinel draw after the call).

  * plan parity (host only): reseeding and calling `.plan` gives the recorded decisions, patches, tubes and proposals BIT FOR BIT and
    leaves numpy's stream where the reference left it;
  * `np_apply`: a numpy restatement of the pixel pipeline, written stage by stage on whole frames as the reference runs it (NOT as the
    kernel's gather), reproduces the recorded output bit for bit -- the host-side pin, no kernel involved;
  * kernel cases: step_clip_augment_u8's fp32 output is bit-equal to the fixture, its bf16 / fp16 output to the round-to-nearest-even of
    that, with the rgb swap, per-clip source sizes in one batch, the identity plan against step_clip_from_u8, and bad arguments;
  * module cases: `.plan` + `.apply` on a batch (tensor input, list input, `out=`).
All equalities are exact: every stage is a fixed sequence of float32 operations, and the issue of rounding order is settled by the
fixture, so no tolerance exists to choose."""
import ctypes

import numpy as np

from step_amd import _capi
from step_amd.augment import AugPlan, BaseTransform, TubeAugmentation
from tests.kernel_cases import to_bf16_bits

F32, BF16, F16 = _capi.F32, _capi.BF16, _capi.F16
f32 = np.float32
EPS = f32(1.1920928955078125e-7)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def case_names(g):
    return [str(n) for n in g["cases"]]


def load_case(g, name):
    k = name + "_"
    c = dict(name=name, seed=int(g[k + "seed"]), base=bool(g[k + "kind"]), size=tuple(int(v) for v in g[k + "size"]), scale=int(g[k + "scale"]),
             mean=tuple(g[k + "mean"].tolist()), stds=tuple(g[k + "stds"].tolist()), frames=g[k + "frames"], out=g[k + "out"],
             sentinel=float(g[k + "sentinel"]), crop=tuple(int(v) for v in g[k + "crop"]), mirror=bool(g[k + "mirror"]), photo=g[k + "photo"],
             params=g[k + "params"], perm=tuple(int(v) for v in g[k + "perm"]), rects=g[k + "rects"], patches=g[k + "patches"])
    c["switches"] = dict(zip(("do_flip", "do_crop", "do_photometric", "do_erase"), (bool(v) for v in g[k + "switches"])))
    for n in ("tubes_in", "tubes_out", "props_in", "props_out"):
        c[n] = g[k + n] if k + n in g.files else None
    return c


def transform_of(c):
    if c["base"]:
        return BaseTransform(c["size"], c["mean"], c["stds"], scale=c["scale"])
    return TubeAugmentation(c["size"], c["mean"], c["stds"], scale=c["scale"], **c["switches"])


def recorded_plan(c):
    """The AugPlan the fixture's observed decisions describe (built from the record, not by `.plan`)."""
    T, H, W, _ = c["frames"].shape
    p = AugPlan(H, W)
    p.crop, p.mirror, p.perm = c["crop"], c["mirror"], c["perm"]
    on = c["photo"]
    p.photometric, p.contrast_first = bool(on[0]), bool(on[3])
    p.brightness = f32(c["params"][0]) if on[1] else None
    p.contrast = f32(c["params"][1]) if on[2] else None
    p.saturation = f32(c["params"][2]) if on[4] else None
    p.hue = f32(c["params"][3]) if on[5] else None
    at = 0
    for x1, y1, x2, y2 in c["rects"].tolist():
        n = (y2 - y1) * (x2 - x1) * 3
        p.rects.append((x1, y1, x2, y2))
        p.patches.append(c["patches"][at:at + n].reshape(y2 - y1, x2 - x1, 3))
        at += n
    assert at == c["patches"].size
    return p


def seeded_plan(c):
    np.random.seed(c["seed"])
    shape = c["frames"].shape[:3]
    return transform_of(c).plan(shape, c["tubes_in"], c["props_in"])


def same_plan(a, b):
    def eq(x, y):
        return (x is None and y is None) or (x is not None and y is not None and f32(x).tobytes() == f32(y).tobytes())
    return ((a.Hs, a.Ws, tuple(a.crop), a.mirror, a.photometric, tuple(a.perm)) == (b.Hs, b.Ws, tuple(b.crop), b.mirror, b.photometric, tuple(b.perm))
            and (not a.photometric or a.contrast_first == b.contrast_first)
            and all(eq(getattr(a, n), getattr(b, n)) for n in ("brightness", "contrast", "saturation", "hue"))
            and [tuple(r) for r in a.rects] == [tuple(r) for r in b.rects]
            and len(a.patches) == len(b.patches) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a.patches, b.patches)))


def same_array(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_plan_parity(golden):
    g = golden("augment_golden")
    for name in case_names(g):
        c = load_case(g, name)
        tubes_before = None if c["tubes_in"] is None else c["tubes_in"].copy()
        plan, tubes, props = seeded_plan(c)
        sentinel = np.random.random_sample()
        assert same_plan(plan, recorded_plan(c)), name
        assert same_array(tubes, c["tubes_out"]), name
        assert same_array(props, c["props_out"]), name
        assert sentinel == c["sentinel"], (name, "the RNG stream is not where the reference left it")
        assert same_array(tubes_before, c["tubes_in"]), (name, "plan() modified its input")


# ---- the numpy restatement of the pixel pipeline -------------------------------------------------------------------------------------
def _to_hsv(x):
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = diff / (np.abs(v) + EPS)
    d = (60. / (diff + EPS).astype(np.float64)).astype(f32)
    h = np.where(v == r, (g - b) * d, np.where(v == g, (b - r) * d + f32(120), (r - g) * d + f32(240)))
    h = np.where(h < 0, h + f32(360), h)
    return np.stack([h, s, v], -1).astype(f32)


def _from_hsv(x):
    h, s, v = x[..., 0], x[..., 1], x[..., 2]
    one = f32(1)
    h = h * (f32(6) / f32(360))
    h = np.where(h < 0, h + f32(6), np.where(h >= 6, h - f32(6), h))
    sector = np.floor(h)
    h = h - sector
    sector = sector.astype(np.int64)
    bad = (sector < 0) | (sector > 5)
    sector, h = np.where(bad, 0, sector), np.where(bad, f32(0), h)
    t = [v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))]
    pick = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))
    chans = []
    for c in range(3):
        acc = np.zeros_like(v)
        for k in range(6):
            acc = np.where(sector == k, t[pick[k][c]], acc)
        chans.append(np.where(s == 0, v, acc))
    return np.stack(chans, -1).astype(f32)


def _axis(dst, src):
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (float(src) / dst) - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(f32)).astype(f32)
    f[(s < 0) | (s >= src - 1)] = 0
    s = np.clip(s, 0, src - 1)
    return s, np.minimum(s + 1, src - 1), f


def np_apply(frames, plan, size, scale=2, mean=(0, 0, 0), stds=(1, 1, 1)):
    """uint8 BGR frames [T,H,W,3] + AugPlan -> the float32 [T,Ho,Wo,3] image the reference's transform returns (BGR order; the
    (2,1,0) swap of data/ava.py:335 and the permute come after it).  Whole-frame stages in the reference's order."""
    Wo, Ho = size
    with np.errstate(all="ignore"):
        x = frames.astype(f32)
        if plan.photometric:
            if plan.brightness is not None:
                x = x + f32(plan.brightness)
            if plan.contrast is not None and plan.contrast_first:
                x = x * f32(plan.contrast)
            x = _to_hsv(x)
            if plan.saturation is not None:
                x[..., 1] = x[..., 1] * f32(plan.saturation)
            if plan.hue is not None:
                h = x[..., 0] + f32(plan.hue)
                h = np.where(h > 360, h - f32(360), h)
                x[..., 0] = np.where(h < 0, h + f32(360), h)
            x = _from_hsv(x)
            if plan.contrast is not None and not plan.contrast_first:
                x = x * f32(plan.contrast)
            x = x[..., list(plan.perm)]
        if scale == 1:
            x = x / f32(255)
        elif scale == 2:
            x = np.clip(x, 0, 255) * f32(2) / f32(255) - f32(1)
        cx, cy, cw, ch = plan.crop
        x = x[:, cy:cy + ch, cx:cx + cw]
        if plan.mirror:
            x = x[:, :, ::-1]
        x = np.array(x, dtype=f32)
        for (x1, y1, x2, y2), patch in zip(plan.rects, plan.patches):
            x[:, y1:y2, x1:x2] = patch
        if (cw, ch) != (Wo, Ho):
            x0, x1, fx = _axis(Wo, cw)
            y0, y1, fy = _axis(Ho, ch)
            fx, fy = fx[None, None, :, None], fy[None, :, None, None]
            one = f32(1)
            top = x[:, y0][:, :, x0] * (one - fx) + x[:, y0][:, :, x1] * fx
            bot = x[:, y1][:, :, x0] * (one - fx) + x[:, y1][:, :, x1] * fx
            x = top * (one - fy) + bot * fy
        x = (x - np.array(mean, f32)) / np.array(stds, f32)
    assert x.dtype == f32
    return np.ascontiguousarray(x)


def check_numpy_restatement(golden):
    g = golden("augment_golden")
    for name in case_names(g):
        c = load_case(g, name)
        got = np_apply(c["frames"], recorded_plan(c), c["size"], c["scale"], c["mean"], c["stds"])
        assert same_array(got, c["out"]), (name, float(np.abs(got - c["out"]).max()))


# ---- driving the C ABI ---------------------------------------------------------------------------------------------------------------
def _addr(ptr):
    return ptr.value if isinstance(ptr, ctypes.c_void_p) else int(ptr)


def pack_block(plans, addrs):
    """include/step_amd.h's plan block as a uint8 array: step_aug_clip[N] | step_aug_rect[] | patches (4-byte words)."""
    N = len(plans)
    n_rects = sum(len(p.rects) for p in plans)
    words = 16 * N + 6 * n_rects + sum(q.size for p in plans for q in p.patches)
    blk = np.zeros(4 * max(words, 4), np.uint8)
    i32, fl = blk.view(np.int32), blk.view(np.float32)
    rect_at, patch_at = 16 * N, 16 * N + 6 * n_rects
    for n, (p, a) in enumerate(zip(plans, addrs)):
        o = 16 * n
        blk[4 * o:4 * o + 8].view(np.uint64)[0] = a
        i32[o + 2:o + 10] = (p.Hs, p.Ws) + tuple(p.crop) + (p.flags(), p.perm[0] | p.perm[1] << 2 | p.perm[2] << 4)
        fl[o + 10:o + 14] = [0 if v is None else v for v in (p.brightness, p.contrast, p.saturation, p.hue)]
        i32[o + 14:o + 16] = (len(p.rects), rect_at)
        for r, q in zip(p.rects, p.patches):
            i32[rect_at:rect_at + 6] = tuple(r) + (patch_at, 0)
            fl[patch_at:patch_at + q.size] = q.reshape(-1)
            rect_at, patch_at = rect_at + 6, patch_at + q.size
    return blk


def run_kernel(bk, clips, plans, size, scale, mean, stds, rgb=False, dtype=F32):
    """clips: list of uint8 [T,H,W,3]; returns the [N,T,3,Ho,Wo] output (fp32, or the 16-bit patterns as uint16)."""
    Wo, Ho = size
    T = clips[0].shape[0]
    src = [bk.dev(c) for c in clips]
    block = bk.dev(pack_block(plans, [_addr(s.ptr) for s in src]))
    out = bk.dev(np.zeros((len(clips), T, 3, Ho, Wo), np.float32 if dtype == F32 else np.uint16))
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_float * 3)(*[float(v) for v in stds])
    rc = bk.lib.step_clip_augment_u8(block.ptr, len(clips), T, Ho, Wo, scale, m, sd, int(rgb), dtype, out.ptr, bk.stream)
    assert rc == 0, rc
    return out.get()


def nchw(x, rgb=False):
    """[T,Ho,Wo,3] -> [T,3,Ho,Wo], with data/ava.py:335's channel swap first when rgb."""
    return np.ascontiguousarray(np.transpose(x[..., ::-1] if rgb else x, (0, 3, 1, 2)))


def case_kernel_fixture_fp32(bk, golden):
    """Every fixture case: fp32 output bit-equal to the reference's, without and with the rgb swap."""
    g = golden("augment_golden")
    for name in case_names(g):
        c = load_case(g, name)
        for rgb in (False, True):
            got = run_kernel(bk, [c["frames"]], [recorded_plan(c)], c["size"], c["scale"], c["mean"], c["stds"], rgb=rgb)
            assert same_array(got[0], nchw(c["out"], rgb)), (name, rgb, float(np.abs(got[0] - nchw(c["out"], rgb)).max()))


def case_kernel_fixture_16bit(bk, golden):
    """bf16 / fp16 output == round-to-nearest-even of the fp32 result, every case (widths 32 and 40: whole 16-byte runs)."""
    g = golden("augment_golden")
    for name in case_names(g):
        c = load_case(g, name)
        want = nchw(c["out"], True)
        for dt, bits in ((BF16, to_bf16_bits(want)), (F16, want.astype(np.float16).view(np.uint16))):
            got = run_kernel(bk, [c["frames"]], [recorded_plan(c)], c["size"], c["scale"], c["mean"], c["stds"], rgb=True, dtype=dt)
            assert np.array_equal(got[0], bits), (name, dt)


def case_kernel_mixed_batch(bk, golden):
    """One launch over clips whose source sizes, crops and plans differ (the cases that share output size, scale, mean and std)."""
    g = golden("augment_golden")
    cs = [load_case(g, n) for n in case_names(g)]
    groups = {}
    for c in cs:
        groups.setdefault((c["size"], c["scale"], c["mean"], c["stds"]), []).append(c)
    sizes = 0
    for (size, scale, mean, stds), grp in groups.items():
        got = run_kernel(bk, [c["frames"] for c in grp], [recorded_plan(c) for c in grp], size, scale, mean, stds, rgb=True)
        for k, c in enumerate(grp):
            assert same_array(got[k], nchw(c["out"], True)), c["name"]
        sizes = max(sizes, len(set(c["frames"].shape for c in grp)))
    assert sizes >= 3                                                         # at least three different source sizes in one launch


def case_kernel_ragged_width(bk, golden):
    """An output width that is no multiple of 8 (the scalar-store form with its partial last run) against np_apply, which the fixture
    pins: all-four plans drawn by TubeAugmentation."""
    rs = np.random.RandomState(5)
    frames = rs.randint(0, 256, (2, 30, 44, 3)).astype(np.uint8)
    tubes = np.tile(np.array([[[0.2, 0.2, 0.8, 0.9]], [[0.3, 0.1, 0.9, 0.7]]], f32), (1, 2, 1))
    aug = TubeAugmentation((27, 21), (0.1, 0.2, 0.3), (0.9, 1.1, 1.2), True, True, True, True, scale=2)
    for seed in (1, 2, 3, 4):
        np.random.seed(seed)
        plan, _, _ = aug.plan(frames.shape[:3], tubes)
        want = nchw(np_apply(frames, plan, aug.size, 2, aug.mean, aug.stds))
        got = run_kernel(bk, [frames], [plan], aug.size, 2, aug.mean, aug.stds)
        assert same_array(got[0], want), seed
        got16 = run_kernel(bk, [frames], [plan], aug.size, 2, aug.mean, aug.stds, dtype=BF16)
        assert np.array_equal(got16[0], to_bf16_bits(want)), seed


def case_kernel_identity_is_clip_from_u8(bk, golden):
    """An identity plan at the network's resolution == step_clip_from_u8, every dtype and scale (rgb off: the ingest does not swap)."""
    rs = np.random.RandomState(9)
    N, T, H, W = 2, 3, 12, 24
    fr = rs.randint(0, 256, (N, T, H, W, 3)).astype(np.uint8)
    mean, stds = (0.1, -0.2, 0.3), (1.0, 0.5, 2.0)
    m = (ctypes.c_float * 3)(*mean)
    sd = (ctypes.c_float * 3)(*stds)
    src = bk.dev(fr)
    for scale in (0, 1, 2):
        for dt, z in ((F32, np.float32), (BF16, np.uint16), (F16, np.uint16)):
            ref = bk.dev(np.zeros((N, T, 3, H, W), z))
            assert bk.lib.step_clip_from_u8(src.ptr, N, T, H, W, scale, m, sd, dt, ref.ptr, bk.stream) == 0
            got = run_kernel(bk, [fr[0], fr[1]], [AugPlan(H, W), AugPlan(H, W)], (W, H), scale, mean, stds, dtype=dt)
            assert np.array_equal(got, ref.get()), (scale, dt)


def case_kernel_bad_arguments(bk, golden):
    fr = np.zeros((1, 4, 8, 3), np.uint8)
    src = bk.dev(fr)
    block = bk.dev(pack_block([AugPlan(4, 8)], [_addr(src.ptr)]))
    out = bk.dev(np.zeros((1, 1, 3, 4, 8), np.float32))
    call = bk.lib.step_clip_augment_u8
    assert call(block.ptr, 1, 1, 4, 8, 2, None, None, 0, F32, out.ptr, bk.stream) == 0
    assert call(block.ptr, -1, 1, 4, 8, 2, None, None, 0, F32, out.ptr, bk.stream) == -2          # STEP_E_SHAPE
    assert call(block.ptr, 1, 0, 4, 8, 2, None, None, 0, F32, out.ptr, bk.stream) == -2
    assert call(block.ptr, 1, 1, 0, 8, 2, None, None, 0, F32, out.ptr, bk.stream) == -2
    assert call(block.ptr, 1, 1, 4, 8, 3, None, None, 0, F32, out.ptr, bk.stream) == -2
    assert call(block.ptr, 1, 1, 4, 8, 2, None, None, 0, 7, out.ptr, bk.stream) == -1             # STEP_E_DTYPE
    assert call(None, 1, 1, 4, 8, 2, None, None, 0, F32, out.ptr, bk.stream) == -3                # STEP_E_NULL
    assert call(block.ptr, 1, 1, 4, 8, 2, None, None, 0, F32, None, bk.stream) == -3
    assert call(_addr(block.ptr) + 4, 1, 1, 4, 8, 2, None, None, 0, F32, out.ptr, bk.stream) == -5  # STEP_E_ALIGN
    assert call(None, 0, 1, 4, 8, 2, None, None, 0, F32, None, bk.stream) == 0                    # an empty batch is no error


KERNEL_CASES = ["case_kernel_fixture_fp32", "case_kernel_fixture_16bit", "case_kernel_mixed_batch", "case_kernel_ragged_width",
                "case_kernel_identity_is_clip_from_u8", "case_kernel_bad_arguments"]


# ---- the module ------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    import torch

    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16) if t.dtype in (torch.bfloat16, torch.float16) else t.detach().cpu().numpy()


def module_batch_matches_fixture(device, golden):
    """TubeAugmentation.plan + .apply on a batch == the per-clip fixture outputs stacked: list input (source sizes differ), fp32 and
    bf16, rgb on and off."""
    import torch

    g = golden("augment_golden")
    grp = [load_case(g, n) for n in ("A", "F", "L")]                          # one output size, scale, mean and std; three source sizes
    assert len(set((c["size"], c["scale"], c["mean"], c["stds"]) for c in grp)) == 1 and len(set(c["frames"].shape for c in grp)) == 3
    aug = TubeAugmentation(grp[0]["size"], grp[0]["mean"], grp[0]["stds"], True, True, True, True, scale=grp[0]["scale"])
    plans = []
    for c in grp:
        plan, tubes, props = seeded_plan(c)                                    # (each case's own switches drew its plan)
        assert same_array(tubes, c["tubes_out"]) and same_array(props, c["props_out"])
        plans.append(plan)
    clips = [torch.from_numpy(c["frames"]).to(device) for c in grp]
    for rgb in (True, False):
        want = np.stack([nchw(c["out"], rgb) for c in grp])
        got = aug.apply(clips, plans, dtype=torch.float32, rgb=rgb)
        assert tuple(got.shape) == want.shape and np.array_equal(_bits(got), want), rgb
    got = aug.apply(clips, plans)                                              # the default: bf16, rgb
    assert got.dtype == torch.bfloat16 and np.array_equal(_bits(got), to_bf16_bits(np.stack([nchw(c["out"], True) for c in grp])))


def module_tensor_input_and_out(device, golden):
    """One [N,T,Hs,Ws,3] tensor as input, `out=` filled in place (its dtype wins), BaseTransform drawing nothing."""
    import torch

    g = golden("augment_golden")
    c = load_case(g, "I")
    aug = transform_of(c)
    state = np.random.get_state()[1].copy()
    plan, tubes, props = aug.plan(c["frames"].shape[:3], c["tubes_in"], c["props_in"])
    assert np.array_equal(np.random.get_state()[1], state)                     # BaseTransform.plan draws nothing
    assert same_plan(plan, recorded_plan(c)) and same_array(tubes, c["tubes_out"]) and same_array(props, c["props_out"])
    batch = torch.from_numpy(np.stack([c["frames"], c["frames"][::-1].copy()])).to(device)
    want = np.stack([nchw(c["out"], True), nchw(c["out"][::-1], True)])
    out = torch.full((2, c["frames"].shape[0], 3, c["size"][1], c["size"][0]), 7.0, dtype=torch.float16, device=device)
    ret = aug.apply(batch, [plan, plan], dtype=torch.float32, out=out)
    assert ret is out and np.array_equal(_bits(out), want.astype(np.float16).view(np.uint16))
    assert np.array_equal(_bits(aug.apply(batch, [plan, plan], dtype=torch.float32)), want)


def module_refuses_bad_input(device, golden):
    import pytest
    import torch

    aug = BaseTransform((8, 8), scale=2)
    fr = torch.zeros((1, 2, 6, 10, 3), dtype=torch.uint8, device=device)
    plan = aug.plan((2, 6, 10))[0]
    with pytest.raises(RuntimeError):
        aug.apply(fr.float(), [plan])
    with pytest.raises(RuntimeError):
        aug.apply(fr, [plan, plan])
    with pytest.raises(RuntimeError):
        aug.apply(fr, [aug.plan((2, 6, 12))[0]])                               # a plan drawn for another frame size
    with pytest.raises(RuntimeError):
        aug.apply(fr, [plan], out=torch.zeros((1, 2, 3, 8, 9), device=device))
    bad = aug.plan((2, 6, 10))[0]
    bad.crop = (4, 0, 8, 6)                                                    # leaves the frame: refused on the host, never launched
    with pytest.raises(ValueError):
        aug.apply(fr, [bad])


MODULE_CASES = ["module_batch_matches_fixture", "module_tensor_input_and_out", "module_refuses_bad_input"]
