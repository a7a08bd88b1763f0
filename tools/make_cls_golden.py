#!/usr/bin/env python
"""tools/make_cls_golden.py -- writes tests/golden/cls_golden.npz: what the reference's loader samples around ground-truth boxes for the
classification pre-training stage (data/ava_cls.py:200-261 sample_anchors), for both modes and several `random` seeds.

Method: the reference's `data.ava_cls` is imported from where the reference lies at generation time and its function is called as it
stands.  Modules it imports that do not exist here are replaced by empty stand-ins in `sys.modules` BEFORE the import (`cv2`, and whatever
else of its import chain is missing: none of them is touched by sample_anchors), and `np.float`, which numpy 2 no longer has, is set to the
builtin it used to alias.  No reference code is copied.

Cases (boxes normalised to [0, 1], float64 -- the precision the function's own arithmetic has): an isolated box; two identical boxes (no
trial can overlap one by more than pos_thresh and the other by less than neg_thresh: the fallback to the box itself); a box on the frame
border; a box that nearly fills the frame; and three boxes of one clip.  Per case and seed the file holds the inputs, the arguments, the
seed, the output and the next `random.random()` (so a test can check that the stream is left where the reference leaves it).  Needs the
reference tree; not run by the tests, which read only the .npz.

    python tools/make_cls_golden.py
"""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import OUT, REF  # noqa: E402

BOXES = {
    "isolated": [[0.30, 0.35, 0.55, 0.80]],
    "identical": [[0.20, 0.25, 0.50, 0.70], [0.20, 0.25, 0.50, 0.70]],
    "border": [[0.0, 0.0, 0.22, 0.41], [0.70, 0.55, 1.0, 1.0]],
    "full": [[0.02, 0.03, 0.97, 0.99]],
    "three": [[0.05, 0.10, 0.30, 0.60], [0.40, 0.15, 0.62, 0.75], [0.66, 0.30, 0.93, 0.90]],
}
# (pos_num, neg_ratio, mode): the loader's call (ava_cls.py:352: neg_ratio 3), the defaults, and two positives per box
ARGS = [(1, 3, "train"), (1, 3, "val"), (1, 1, "train"), (2, 2, "train"), (1, 0, "train")]
SEEDS = (0, 1, 2, 3)


class _StandIn(types.ModuleType):
    """an empty module whose every attribute is another one (`from torchvision import transforms` must bind something)"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sub = _StandIn(self.__name__ + "." + name)
        setattr(self, name, sub)
        return sub


def import_reference():
    np.float = float                                                        # (numpy < 1.20's alias, used at ava_cls.py:223,245)
    sys.path.insert(0, REF)
    for _ in range(16):
        try:
            import data.ava_cls as M                                        # reference
            return M
        except ImportError as e:
            name = getattr(e, "name", None)
            if not name or name.split(".")[0] in ("data", "utils"):
                raise
            parts = name.split(".")
            for k in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:k]), _StandIn(".".join(parts[:k])))
            for k in list(sys.modules):
                if k == "data" or k.startswith("data."):
                    del sys.modules[k]
    raise SystemExit("the reference's data.ava_cls does not import")


def main():
    M = import_reference()
    g, names = {}, []
    stats = dict(sampled=0, fallback=0, short=0, cases=0)
    for name, boxes in BOXES.items():
        anchors = np.array(boxes, np.float64)
        for pos_num, neg_ratio, mode in ARGS:
            for seed in SEEDS:
                random.seed(seed)
                out = M.sample_anchors(anchors.copy(), pos_num=pos_num, neg_ratio=neg_ratio, mode=mode)
                nxt = random.random()
                k = "%s_p%d_n%d_%s_s%d" % (name, pos_num, neg_ratio, mode, seed)
                names.append(k)
                g[k + "_in"], g[k + "_args"], g[k + "_mode"] = anchors, np.array([pos_num, neg_ratio, seed], np.int64), np.array(mode)
                g[k + "_out"], g[k + "_next"] = np.asarray(out, np.float64), np.float64(nxt)
                assert out.dtype == np.float64
                stats["cases"] += 1
                if mode == "train":
                    own = [any((out == a).all(axis=1)) for a in anchors]
                    stats["fallback"] += int(any(own))
                    stats["sampled"] += int(not all(own))
                    stats["short"] += int(len(out) < len(anchors) * pos_num * (1 + neg_ratio))
    g["cases"] = np.array(names)
    print("cases %(cases)d: with a sampled positive %(sampled)d, with a fallback to the box itself %(fallback)d, short of the full row count %(short)d" % stats)
    assert stats["sampled"] and stats["fallback"] and stats["short"]
    path = os.path.join(OUT, "cls_golden.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 200000


if __name__ == "__main__":
    main()
