#!/usr/bin/env python
"""tools/make_video_golden.py -- writes tests/golden/video_index_golden.json: which source frames the reference's video loader
(data/customize.py:75-105, CustomizedDataset.read_images) reads for the clip centred on a frame, and the anchor tubes its __getitem__
returns (:129-146).

Method: the reference's `data.customize` is imported from where the reference lies at generation time and its methods are called as
they stand.  `cv2` does not exist here and is replaced in `sys.modules` BEFORE the import by a stand-in whose `imread` returns the frame
NUMBER parsed from the file name, so `read_images` returns the list of frame numbers it would have decoded.  The dataset is built with
`object.__new__` and its attributes are set by hand (its constructor globs a directory of videos).  No reference code is copied.

Recorded: source_fps / target_fps in {30/12, 25/12, 12/12, 10/12} x frames in {36, 12} x (fid, numf) in {(0,50), (1,50), (49,50),
(120,300), (0,1), (3,7)}.  Needs the reference tree; not run by the tests, which read only the .json.

    python tools/make_video_golden.py
"""
import json
import os
import re
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import OUT, REF  # noqa: E402

RATES = ((30, 12), (25, 12), (12, 12), (10, 12))
SHAPES = ((3, 3), (3, 1))                      # (T, chunks): 36 and 12 frames per clip
POINTS = ((0, 50), (1, 50), (49, 50), (120, 300), (0, 1), (3, 7))


def main():
    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda name: int(re.search(r"(\d+)\.jpg$", name).group(1))
    sys.modules["cv2"] = cv2
    sys.path.insert(0, REF)
    from data.customize import TEM_REDUCE, CustomizedDataset

    def dataset(T, chunks, source_fps, target_fps, anchor_mode="1"):
        ds = object.__new__(CustomizedDataset)
        ds.data_root, ds.T, ds.chunks, ds.source_fps, ds.target_fps = "videos", T, chunks, source_fps, target_fps
        ds.stride, ds.anchor_mode, ds.im_format = 1, anchor_mode, "frame%04d.jpg"
        ds.transform = lambda images: (np.zeros((len(images), 1, 1, 3), np.float32), None, None)
        return ds

    cases = []
    for source_fps, target_fps in RATES:
        for T, chunks in SHAPES:
            ds = dataset(T, chunks, source_fps, target_fps)
            for fid, numf in POINTS:
                idx = [int(v) for v in ds.read_images("v", fid, numf)]
                assert len(idx) == T * chunks * TEM_REDUCE
                cases.append(dict(source_fps=source_fps, target_fps=target_fps, T=T, chunks=chunks, frames=len(idx), fid=fid, numf=numf, indices=idx))
    tubes = {}
    for mode in ("1", "0"):
        ds = dataset(3, 3, 30, 12, mode)
        ds.data = [("v", 5, 50)]
        _, anchor_tubes, info = ds[0]
        assert info == {"video_name": "v", "fid": 5}
        tubes[mode] = dict(shape=list(anchor_tubes.shape), values=[float(v) for v in np.asarray(anchor_tubes, np.float64).reshape(-1)])
    path = os.path.join(OUT, "video_index_golden.json")
    with open(path, "w") as f:
        json.dump(dict(cases=cases, anchor_tubes=tubes), f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d index lists, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
