"""tools/roi_bwd_bench.py -- ROIAlign backward (fixed-order gather | atomics) at the training step's shapes (GPU only, tuning aid)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from step_amd import _lib, ops  # noqa: E402
from step_amd.tube_math import generate_anchors  # noqa: E402
from tools import abkit  # noqa: E402

for clips, tubes, Tl in ((1, 5, 9), (8, 15, 3), (8, 15, 9), (8, 34, 9)):
    a = torch.from_numpy(generate_anchors()[:tubes] * 400.0).float()
    rois = []
    for b in range(clips):
        for k in range(tubes):
            for t in range(Tl):
                rois.append([b * Tl + t] + a[k].tolist())
    rois = torch.tensor(rois, device="cuda")
    K = rois.shape[0]
    g = torch.randn(K, 7, 7, 832, device="cuda").permute(0, 3, 1, 2)
    out = {}
    libs = {"cur": _lib.lib()}
    try:
        libs["prev"] = abkit.load_build("prev")                # (the parent's library, where tools/build_prev.sh has built it)
    except FileNotFoundError:
        pass
    for nm, L_ in libs.items():
        with _lib.use(L_):
            print("   lib=%s gather %.3f ms" % (nm, abkit.wall_ms(lambda: ops.roi_align_backward(g, rois, 7, 7, 1 / 16., 0, clips * Tl, 832, 25, 25), 5, warm=1)))
    for det in (True, False):
        r = ops.roi_align_backward(g, rois, 7, 7, 1 / 16., 0, clips * Tl, 832, 25, 25, deterministic=det)
        out[det] = (abkit.wall_ms(lambda: ops.roi_align_backward(g, rois, 7, 7, 1 / 16., 0, clips * Tl, 832, 25, 25, deterministic=det), 5), r)
    err = float((out[True][1] - out[False][1]).abs().max() / out[False][1].abs().max())
    print("clips %d tubes %2d Tl %d  K %5d:  gather %.3f ms   atomics %.3f ms   (max rel diff %.1e)" % (clips, tubes, Tl, K, out[True][0], out[False][0], err))
