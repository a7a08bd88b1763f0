"""Cases for the tube growth outside temporal_mode "predict" (step_tube_update_mode, step_tube_grow, step_amd.ops.tube_update_mode /
tube_grow, the "extrapolate" / "mean" branches of driver.inference_flat and selection.DeviceSelector), driven on the host interpreter by
tests/test_emul_tubemode.py and on the real library by tests/test_gpu_tubemode.py.

The reference of the growth is numpy: step_amd.tube_math.extrapolate_tubes (pinned bit for bit to the reference's own output by
inference_modes_golden.npz: ext_in -> ext_out_T3 / ext_out_T6) and np.mean + np.tile + np.concatenate as utils/utils.py:116-118 writes them.
Everything behind the decode is compared for EQUALITY: the growth is products, differences and sums in a fixed order, each rounded on its
own.  The decode itself (one expf per size) is held to 2e-6 * max(1, |ref|), the bound tests/kernel_cases.py case_tube_update uses, and the
growth of a step is then checked against the numpy growth of the KERNEL'S OWN pred_loc: the recurrence amplifies a last-bit difference.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda")."""
import copy

import numpy as np
import torch

from step_amd import tube_math as TM

f32 = np.float32
E_SHAPE, E_NULL, E_UNSUPPORTED = -2, -3, -4
EXTRAPOLATE, MEAN = 1, 2
MODES = {"extrapolate": EXTRAPOLATE, "mean": MEAN}
ALL_MODES = ("predict", "extrapolate", "mean")


# ---- the numpy growth ------------------------------------------------------------------------------------------------------------------
def np_grow(x, Tw, mode):
    """[n,T,4] fp32 -> [n,T+2Tw,4]: tube_utils.py:159-176 / utils.py:114-118"""
    x = np.ascontiguousarray(x, f32)
    if mode in (EXTRAPOLATE, "extrapolate"):
        return TM.extrapolate_tubes(x, Tw)
    m = np.tile(np.mean(x, axis=1, keepdims=True), (1, Tw, 1))
    return np.concatenate((m, x, m), axis=1)


def with_index(prop, clip_of):
    """flatten_tubes' index column in front: clip * Tn + t"""
    n, Tn = prop.shape[:2]
    idx = np.asarray(clip_of, f32).reshape(n, 1, 1) * f32(Tn) + np.arange(Tn, dtype=f32).reshape(1, Tn, 1)
    return np.concatenate((np.broadcast_to(idx, (n, Tn, 1)), prop), axis=2).astype(f32)


def wild_boxes(rs, N, T):
    """boxes as case_tube_update draws them: some degenerate, some outside the frame"""
    xy = rs.uniform(-30, 380, (N, T, 2))
    return np.concatenate([xy, xy + rs.uniform(-2, 160, (N, T, 2))], 2).astype(f32)


# ---- driving the C ABI -----------------------------------------------------------------------------------------------------------------
def grow_call(bk, boxes, Tw, mode, clip_of=None, mask=None, pad=None, validate=0, W=400.0, H=400.0, ext=(400.0, 400.0), expect=0):
    """one step_tube_grow call -> out [N,Tn,5] (pre-filled with 7: every slot is seen to be written), or the status when expect != 0"""
    N, T, cols = boxes.shape
    Tn = T + 2 * Tw
    clip_of = np.zeros(N, np.int32) if clip_of is None else np.asarray(clip_of, np.int32)
    d = [bk.dev(np.ascontiguousarray(boxes, f32)), bk.dev(clip_of), bk.dev(None if mask is None else np.asarray(mask, f32)),
         bk.dev(None if pad is None else np.ascontiguousarray(pad, f32))]
    out = bk.dev(np.full((max(N, 1), max(Tn, 1), 5), 7.0, f32))
    rc = bk.lib.step_tube_grow(d[0].ptr, cols, N, T, Tw, mode, ext[0], ext[1], d[1].ptr, d[2].ptr, d[3].ptr, validate, W, H, out.ptr, bk.stream)
    assert rc == expect, (rc, expect)
    got = out.get().copy()
    if expect != 0:
        assert np.all(got == 7), "a refused call wrote something"
        return rc
    return got[:N]


def update_call(bk, tubes, loc, clip_of, mode, extend, Tw, W, H, expect=0):
    """one step_tube_update_mode call -> (pred_loc, next_tubes)"""
    N, T = tubes.shape[:2]
    Tn = T + 2 * Tw if extend else T
    d = [bk.dev(tubes), bk.dev(loc), bk.dev(np.asarray(clip_of, np.int32))]
    o = [bk.dev(np.full((N, T, 4), 7.0, f32)), bk.dev(np.full((N, Tn, 5), 7.0, f32))]
    rc = bk.lib.step_tube_update_mode(d[0].ptr, N, T, d[1].ptr, d[2].ptr, mode, extend, Tw, 400.0, 400.0, W, H, o[0].ptr, o[1].ptr, bk.stream)
    assert rc == expect, (rc, expect)
    return o[0].get().copy(), o[1].get().copy()


# ---- kernel cases ------------------------------------------------------------------------------------------------------------------------
def case_grow_extrapolate_golden(bk, golden):
    """the reference's own extrapolate_tubes output, clamps at 0 and 399 included, bit for bit: T = Tw = 3 and T = Tw = 6.  A contracted
    (FMA) or re-associated recurrence differs in about a third of the unclamped values of ext_out_T6."""
    g = golden("inference_modes_golden")
    x = g["ext_in"]
    for boxes, Tw, want in ((x, 3, g["ext_out_T3"]), (np.tile(x, (1, 2, 1)), 6, g["ext_out_T6"])):
        assert np.array_equal(np_grow(boxes, Tw, EXTRAPOLATE), want)                          # (the numpy form the other cases lean on)
        got = grow_call(bk, boxes, Tw, EXTRAPOLATE)
        assert got.shape == (7, boxes.shape[1] + 2 * Tw, 5)
        bad = np.argwhere(got[..., 1:] != want)
        assert np.array_equal(got[..., 1:], want), (Tw, len(bad), bad[:4].tolist())
        assert (want == 0).any() and (want == 399).any()
        assert np.array_equal(got[..., 0], np.broadcast_to(np.arange(got.shape[1], dtype=f32), got.shape[:2]))


def case_grow_mean(bk, golden):
    """np.mean(axis=1) of fp32 boxes, tiled Tw times on both sides: T = 3 and T = 9"""
    rs = np.random.RandomState(31)
    for T in (3, 9):
        x = rs.uniform(0, 400, (5, T, 4)).astype(f32)
        got = grow_call(bk, x, 3, MEAN)
        want = np_grow(x, 3, MEAN)
        assert got.shape == (5, T + 6, 5) and np.array_equal(got[..., 1:], want), (T, np.argwhere(got[..., 1:] != want)[:4].tolist())


def case_grow_mask_pad_index(bk, golden):
    """7 rows over 3 clips, five columns per box (the first ignored), rows 2 and 5 masked: the clip's pad exactly, column 0 = clip * Tn + t
    on every row; validate = 1 on degenerate and outside boxes and one NaN coordinate against tube_math.valid_tubes of the numpy growth
    (the NaN box becomes the whole frame); validate = 0 leaves the NaN a NaN."""
    rs = np.random.RandomState(32)
    N, T, Tw = 7, 3, 3
    Tn = T + 2 * Tw
    clip_of = np.array([0, 0, 0, 1, 2, 2, 2], np.int32)
    mask = np.array([1, 1, 0, 1, 1, 0, 1], f32)
    pad = rs.uniform(0, 300, (3, Tn, 4)).astype(f32)
    box = wild_boxes(rs, N, T)
    box[4, 1, 2] = np.nan
    rows = np.concatenate([rs.uniform(0, 50, (N, T, 1)).astype(f32), box], 2)
    W, H = 320.0, 240.0
    for name, mode in MODES.items():
        grown = np_grow(box, Tw, mode)
        assert np.isnan(grown[4]).any() and not np.isnan(np.delete(grown, 4, axis=0)).any()
        for validate in (0, 1):
            got = grow_call(bk, rows, Tw, mode, clip_of, mask, pad, validate, W, H)
            want = TM.valid_tubes(grown, W, H) if validate else grown.copy()
            want[mask == 0] = pad[clip_of[mask == 0]]
            assert np.array_equal(got[..., 0], with_index(want, clip_of)[..., 0]), (name, validate)
            assert np.array_equal(got[..., 1:], want, equal_nan=True), (name, validate, np.argwhere(got[..., 1:] != want)[:4].tolist())
            if validate:
                assert not np.isnan(got).any() and np.array_equal(got[4, 1, 1:], np.array([0, 0, W, H], f32))
            else:
                assert np.array_equal(np.isnan(got[..., 1:]), np.isnan(grown)) and np.isnan(got[4, 1, 3])
        # four columns, no mask: the same boxes
        got4 = grow_call(bk, box, Tw, mode, clip_of)
        assert np.array_equal(got4[..., 1:], grown, equal_nan=True) and np.array_equal(got4[..., 0], with_index(grown, clip_of)[..., 0])


UPDATE_SHAPES = ((7, 3, 3, 1), (5, 9, 3, 0), (4, 9, 3, 1), (1, 3, 3, 0), (300, 3, 3, 1))           # (the last crosses workgroups)


def case_update_mode(bk, golden):
    """step_tube_update_mode, both modes: pred_loc against tube_math.decode_coef within 2e-6 * max(1, |ref|) (expf is the only operation
    whose last bit may differ between libraries); next_tubes bit-equal to numpy growth + valid_tubes + index column of the kernel's OWN
    pred_loc."""
    rs = np.random.RandomState(33)
    W, H = 400.0, 320.0
    for name, mode in MODES.items():
        for N, T, Tw, extend in UPDATE_SHAPES:
            boxes = wild_boxes(rs, N, T)
            tubes = np.concatenate([rs.uniform(0, 50, (N, T, 1)).astype(f32), boxes], 2)
            loc = (rs.randn(N, T, 4) * 0.2).astype(f32)
            clip_of = np.sort(rs.randint(0, 3, N)).astype(np.int32)
            pl, nxt = update_call(bk, tubes, loc, clip_of, mode, extend, Tw, W, H)
            ref = TM.decode_coef(torch.from_numpy(boxes).reshape(-1, 4), torch.from_numpy(loc).reshape(-1, 4)).view(N, T, 4).numpy()
            err, bound = float(np.abs(pl - ref).max()), 2e-6 * max(1.0, float(np.abs(ref).max()))
            print("step_tube_update_mode %s N=%d T=%d extend=%d: pred_loc max err %.3g (bound %.3g)" % (name, N, T, extend, err, bound))
            assert err <= bound, (name, N, T, extend, err, bound)
            want = with_index(TM.valid_tubes(np_grow(pl, Tw, mode) if extend else pl, W, H), clip_of)
            assert nxt.shape == want.shape and np.array_equal(nxt, want), (name, N, T, extend, np.argwhere(nxt != want)[:4].tolist())


def case_errors(bk, golden):
    """the error returns of include/step_amd.h, before any launch; N == 0 is a successful no-op"""
    L, s = bk.lib, bk.stream
    x = np.ones((2, 3, 4), f32)
    assert grow_call(bk, np.ones((2, 60, 4), f32), 3, MEAN, expect=E_UNSUPPORTED) == E_UNSUPPORTED           # 66 frames
    assert grow_call(bk, np.ones((2, 58, 4), f32), 3, MEAN).shape == (2, 64, 5)
    assert grow_call(bk, np.ones((2, 3, 4), f32), 1, EXTRAPOLATE, expect=E_SHAPE) == E_SHAPE                 # Tw - 1 == 0
    assert grow_call(bk, np.ones((2, 3, 4), f32), 1, MEAN).shape == (2, 5, 5)
    assert grow_call(bk, np.ones((2, 3, 4), f32), 4, EXTRAPOLATE, expect=E_SHAPE) == E_SHAPE                 # T < Tw
    assert grow_call(bk, np.ones((2, 3, 4), f32), 4, MEAN).shape == (2, 11, 5)
    for mode in (0, 3, -1):
        assert grow_call(bk, x, 3, mode, expect=E_SHAPE) == E_SHAPE
    assert grow_call(bk, x, 3, MEAN, mask=np.ones(2, f32), expect=E_NULL) == E_NULL                          # a mask without its pad
    assert grow_call(bk, x, 3, MEAN, validate=2, expect=E_SHAPE) == E_SHAPE
    assert L.step_tube_grow(None, 4, 0, 3, 3, EXTRAPOLATE, 400.0, 400.0, None, None, None, 0, 400.0, 400.0, None, s) == 0
    assert L.step_tube_grow(None, 3, 0, 3, 3, EXTRAPOLATE, 400.0, 400.0, None, None, None, 0, 400.0, 400.0, None, s) == E_SHAPE      # box_cols
    assert L.step_tube_grow(None, 4, 2, 3, 3, EXTRAPOLATE, 400.0, 400.0, None, None, None, 0, 400.0, 400.0, None, s) == E_NULL
    upd = lambda N, T, mode, extend, Tw: L.step_tube_update_mode(None, N, T, None, None, mode, extend, Tw, 400.0, 400.0, 400.0, 400.0, None, None, s)
    assert upd(0, 3, EXTRAPOLATE, 1, 3) == 0 and upd(0, 3, MEAN, 0, 3) == 0
    assert upd(2, 60, MEAN, 1, 3) == E_UNSUPPORTED and upd(2, 3, EXTRAPOLATE, 1, 1) == E_SHAPE and upd(2, 3, EXTRAPOLATE, 1, 4) == E_SHAPE
    assert upd(2, 3, 0, 1, 3) == E_SHAPE and upd(2, 3, 3, 0, 3) == E_SHAPE
    assert upd(2, 3, EXTRAPOLATE, 1, 3) == E_NULL


KERNEL_CASES = ["case_grow_extrapolate_golden", "case_grow_mean", "case_grow_mask_pad_index", "case_update_mode", "case_errors"]


# ---- module cases ----------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def case_selector_modes(dev, golden):
    """DeviceSelector(..., temporal_modes=all) under "extrapolate" and "mean", steps 1-3 of the default NUM_CHUNKS, on the inputs of
    select_cases.case_selector_matches_restatement.  Steps 1 and 2 equal the "predict" selector's rows from the same generator state,
    except that step 2 writes no neighbour targets; step 3's sel is the restatement's UN-GROWN rows through the numpy growth where mask = 1
    and the pad elsewhere, its tgt / mask / inv / counts the restatement's; one offset per select(); the positional constructor still
    refuses the mode."""
    import step_amd
    from step_amd import ops
    from step_amd.selection import DeviceSelector
    from tests import select_cases as SC

    tubes, gts = [9, 4, 12], [2, 1, 3]
    for mode in ("extrapolate", "mean"):
        rs = np.random.RandomState(21)
        a = SC.cfg(temporal_mode=mode)
        inp, _, _, flat, hist = SC._module_inputs(rs, tubes, gts, a.num_classes, near=0.7, spread=12)
        for h in hist:                                           # (these modes' histories carry no neighbours)
            h["pred_first_loc"] = h["pred_last_loc"] = None
        rng, rng_p = step_amd.DeviceRNG(dev, seed=41), step_amd.DeviceRNG(dev, seed=41)
        selr = DeviceSelector(a, 3, 15, dev, rng, temporal_modes=ALL_MODES)
        selp = DeviceSelector(SC.cfg(), 3, 15, dev, rng_p)
        gt, gt_count, init_flat, clip_start, pads, dhist = SC._device_args(dev, inp, flat, hist, a)
        clip_of = torch.from_numpy(np.repeat(np.arange(3), tubes).astype(np.int32)).to(dev)
        slot_clip = np.repeat(np.arange(3), 15)
        for step in (1, 2, 3):
            h = dhist[step - 2] if step > 1 else None
            out = selr.select(step, h, gt, gt_count, init_flat, clip_start, pads[step], max_tubes=12)
            assert all(o is s for o, s in zip(out, selr.out[step])) and rng.offset() == step
            got = [_np(t) for t in out]
            if step < 3:
                want = [_np(t) for t in selp.select(step, h, gt, gt_count, init_flat, clip_start, pads[step], max_tubes=12)]
                if step == 2:
                    assert want[1][:, (0, 2)].any() and not got[1][:, (0, 2)].any(), "neighbour targets outside 'predict'"
                    want[1][:, (0, 2)] = 0
                for nm, g_, w_ in zip(SC.NAMES, got, want):
                    assert np.array_equal(g_, w_), (mode, step, nm)
                continue
            score, vloc, _, _, iou = ops.select_prepare(h["pred_prob"], h["pred_loc"], None, None, clip_of, gt[:, :, 1, :4].contiguous(), gt_count,
                                                        400.0, 400.0)
            pad = _np(pads[3])
            r = dict(inp, cand=_np(vloc), score=_np(score), iou=_np(iou), pad=np.ascontiguousarray(pad[:, 3:6]))
            want = SC.restate(r, SC.params(cls_thresh=a.cls_thresh[2], reg_thresh=a.reg_thresh[2]), 41, 2)
            assert want[5] > 1e-9 and want[4].sum() > 10 and not want[2].all()
            real = want[2][:, 0] == 1
            sel = np.empty((45, 9, 4), f32)
            sel[real] = np_grow(want[0][real][:, :, 1:], 3, mode)
            sel[~real] = pad[slot_clip[~real]]
            assert got[0].shape == (45, 9, 5) and np.array_equal(got[0], with_index(sel, slot_clip)), (mode, np.argwhere(got[0][..., 1:] != sel)[:4].tolist())
            for nm, g_, w_ in list(zip(SC.NAMES, got, want))[1:5]:
                assert np.array_equal(g_, w_), (mode, step, nm)
        assert rng.offset() == 3
        try:
            DeviceSelector(a, 3, 15, dev, rng)
        except NotImplementedError:
            pass
        else:
            raise AssertionError("the positional DeviceSelector accepted temporal_mode %r" % (mode,))


def case_selector_modes_agree_with_host(dev, golden):
    """the inputs of select_cases.case_selector_agrees_with_host_selection (no draw decides anything) under "extrapolate":
    selection.train_select and the device selector agree on the positive rows in order and on the SET of negative rows, with their targets,
    at step 3 with nine-frame tubes."""
    import step_amd
    from step_amd.selection import DeviceSelector, train_select
    from tests import select_cases as SC

    rs = np.random.RandomState(22)
    a = SC.cfg(selection_sampling="uniform", temporal_mode="extrapolate")
    B, A, G = 2, 6, 2
    inp, gt_list, init, flat, hist = SC._module_inputs(rs, [A] * B, [G] * B, a.num_classes, near=0.0, spread=2)
    for b in range(B):
        for g in range(G):
            init[b][g] = gt_list[b][g, 1, :4] + rs.uniform(-5, 5, (3, 4)).astype(f32)
        for k in range(G, A):
            box = SC.rand_boxes(rs, 1)[0]
            while max(SC.box_iou_f32(gt_list[b][g, 1, :4], box) for g in range(G)) > 0.05:
                box = SC.rand_boxes(rs, 1)[0]
            init[b][k] = box
        init[b] = np.clip(init[b], 1, 399).astype(f32)
    flat = np.concatenate(init)
    for h in hist:
        h["pred_loc"] = torch.from_numpy((flat + rs.uniform(-2, 2, flat.shape)).astype(f32))
        h["pred_first_loc"] = h["pred_last_loc"] = None
    rng = step_amd.DeviceRNG(dev, seed=43)
    selr = DeviceSelector(a, B, 15, dev, rng, temporal_modes=ALL_MODES)
    gt, gt_count, init_flat, clip_start, pads, dhist = SC._device_args(dev, inp, flat, hist, a)
    step = 3
    h_sel, h_tgt = train_select(step, dhist[1], gt_list, init, a, device=True)
    sel, tgt, mask, _, counts = [_np(t) for t in selr.select(step, dhist[1], gt, gt_count, init_flat, clip_start, pads[step], max_tubes=A)]
    assert sel.shape == (B * 15, 9, 5)
    for b in range(B):
        P, R = int(counts[b, 0]), int(counts[b].sum())
        assert (P, R) == (G, A) == (G, len(h_sel[b])) and h_sel[b].shape == (A, 9, 4), (b, P, R, h_sel[b].shape)
        rows = slice(b * 15, b * 15 + R)
        d_sel, d_tgt = sel[rows][:, :, 1:], tgt[rows]
        assert np.array_equal(d_sel[:P], h_sel[b][:P]) and np.array_equal(d_tgt[:P], h_tgt[b][:P]), (b, "positives")
        key = lambda s_: sorted(range(P, R), key=lambda r: tuple(s_[r].reshape(-1)))
        kd, kh = key(d_sel), key(h_sel[b])
        assert np.array_equal(d_sel[kd], h_sel[b][kh]) and np.array_equal(d_tgt[kd], h_tgt[b][kh]), (b, "negatives")
        assert mask[rows].all() and not mask[b * 15 + R:(b + 1) * 15].any()


MODULE_CASES = ["case_selector_modes", "case_selector_modes_agree_with_host"]


def inference_setup(dev):
    """the networks, feature and tubes of module_cases.case_inference_modes_golden"""
    import step_amd
    from oracle import i3d_ref as R
    from tests import module_cases as MC

    conv_feat = R.fill_tensor("golden.inf.feat", (2, 9, 832, 25, 25), "feat").to(dev)
    conv_cl = conv_feat.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    ctxnet = MC.fill(step_amd.ContextNet(MC.cfg())).to(dev).eval()
    nets = {"roi_net": step_amd.ROINet("align", 7)}
    for i in range(3):
        d = MC.fill(step_amd.TwoBranchNet(MC.cfg()), "det%d." % i).to(dev).eval()
        d.set_device(dev)
        nets["det_net%d" % i] = d
    a = R.anchors()[:11] * 400.0
    tl = [np.tile(a[:, None, :], (1, 3, 1)).astype(f32) for _ in range(2)]
    tl[1] = tl[1][::-1].copy()
    with torch.no_grad():
        ctx = ctxnet(conv_cl)
    return conv_cl, ctx, nets, tl


def case_inference_modes_kernel(dev, golden, mode):
    """driver.inference under `mode` ("extrapolate" | "mean") with TUBE_KERNEL True against False (the tensor-op restatement): the kernel
    form makes three calls of ops.tube_update_mode and none of tube_math.extrapolate_tubes; pred_first_loc is None; pred_loc within the
    decode's 2e-6 bound at step 0 and within the fixture's 1e-3 of inference_modes_golden at every step; every step's pred_prob identical.

    The restatement's "mean" is np.mean's arithmetic (sequential fp32 sum, divided by a device-side divisor), so both modes are bit-identical
    between the two forms at every step (measured on the MI355X: pred_prob and pred_loc max diff 0).  With torch's own `mean`, which multiplies
    the sum by fl(1/3), step 2 under "mean" differed by 3.58e-07 in pred_prob and 1.22e-04 in pred_loc."""
    from step_amd import driver, ops
    from tests import module_cases as MC

    g = golden("inference_modes_golden")
    conv_cl, ctx, nets, tl = inference_setup(dev)
    calls = {"update": 0, "extrapolate": 0}
    real_update, real_ext, real_ext_tm = ops.tube_update_mode, driver.extrapolate_tubes, TM.extrapolate_tubes

    def counted_update(*a, **k):
        calls["update"] += 1
        return real_update(*a, **k)

    def counted_ext(*a, **k):
        calls["extrapolate"] += 1
        return real_ext_tm(*a, **k)

    args = MC.cfg(temporal_mode=mode)
    hists = {}
    for kernel in (True, False):
        calls.update(update=0, extrapolate=0)
        ops.tube_update_mode, driver.extrapolate_tubes, TM.extrapolate_tubes = counted_update, counted_ext, counted_ext
        driver.TUBE_KERNEL = kernel
        try:
            with torch.no_grad():
                hists[kernel], _ = driver.inference(args, conv_cl, ctx, nets, 3, tl)
        finally:
            driver.TUBE_KERNEL = True
            ops.tube_update_mode, driver.extrapolate_tubes, TM.extrapolate_tubes = real_update, real_ext, real_ext_tm
        want = (3, 0) if kernel else (0, 1 if mode == "extrapolate" else 0)
        assert (calls["update"], calls["extrapolate"]) == want, (mode, kernel, calls)
    diffs = []
    for i, (hk, ht) in enumerate(zip(hists[True], hists[False])):
        assert hk["pred_first_loc"] is None and hk["pred_last_loc"] is None
        dp = float((hk["pred_prob"] - ht["pred_prob"]).abs().max())
        dl = float((hk["pred_loc"] - ht["pred_loc"]).abs().max())
        e = MC.rel(_np(hk["pred_loc"]), g["%s_step%d_pred_loc" % (mode, i)])
        ep = MC.rel(_np(hk["pred_prob"][:, 0]), g["%s_step%d_pred_prob" % (mode, i)])
        print("inference %s step %d, kernel vs restatement: pred_prob max diff %.3g, pred_loc max diff %.3g; vs golden rel %.3g / %.3g"
              % (mode, i, dp, dl, e, ep))
        if i == 0:
            ref = _np(ht["pred_loc"])
            assert dl <= 2e-6 * max(1.0, float(np.abs(ref).max())), (mode, dl)
        assert e < 1e-3 and ep < 1e-3, (mode, i, e, ep)
        diffs.append((i, dp, torch.equal(hk["pred_prob"], ht["pred_prob"])))
    assert all(same for _, _, same in diffs), (mode, "pred_prob differs between the kernel and the restatement", diffs)


def case_graphed_inference_extrapolate(dev, golden):
    """GraphedInference under "extrapolate", B = 2, fp32: a replay equals the eager inference_flat bit for bit, and the capacity= form serves
    two different tube counts from ONE capture."""
    from step_amd import driver, workloads

    w = workloads.C3Inference(torch.device(dev), torch.float32, batch=2, tubes=4, graph=False)
    args = copy.copy(w.args)
    args.temporal_mode = "extrapolate"
    rs = np.random.RandomState(3)

    def lists(ns):
        out = []
        for n in ns:
            xy = rs.uniform(10, 250, (n, 1, 2))
            box = np.concatenate([xy, xy + rs.uniform(60, 140, (n, 1, 2))], 2)
            out.append((box + rs.uniform(-4, 4, (n, 3, 4))).astype(f32))
        return out

    keys = ("pred_prob", "pred_loc")
    with torch.no_grad():
        cf = w.base(w.x)
        cx = w.ctx(cf)
        tl = lists((4, 4))
        gi = driver.GraphedInference(args, w.base, w.ctx, w.nets, w.x, tl)
        hist, _, _ = gi()
        flat, nums = driver._flat_tubes(tl, w.x.device)
        clip_of = torch.arange(2, device=w.x.device).repeat_interleave(4)
        eager, _ = driver.inference_flat(args, cf, cx, w.nets, 3, flat, nums, clip_of, want_classes=False)
        assert len(hist) == 3 and hist[2]["pred_loc"].shape[1] == 9
        for i, (a, b) in enumerate(zip(hist, eager)):
            assert a["pred_first_loc"] is None and b["pred_first_loc"] is None
            for k in keys:
                assert torch.equal(a[k], b[k]), ("replay vs eager", i, k)
        del gi
        gc_ = driver.GraphedInference(args, w.base, w.ctx, w.nets, w.x, lists((3, 1)), capacity=4)
        graph = gc_.graph
        for ns in ((3, 1), (2, 4)):
            tl = lists(ns)
            hist, _, _ = gc_(None, tl)
            torch.cuda.synchronize()
            assert gc_.graph is graph and gc_.count.tolist() == list(ns)
            flat, count = driver.pad_tubes(tl, 4, w.x.device, 400, 400)
            eager, _ = driver.inference_flat(args, cf, cx, w.nets, 3, flat, [4, 4], clip_of, want_classes=False, counts=count)
            for i, (a, b) in enumerate(zip(hist, eager)):
                assert a["tubes_count"] is gc_.count and a["pred_first_loc"] is None
                for k in keys:
                    assert torch.equal(a[k], b[k]), (ns, i, k)
