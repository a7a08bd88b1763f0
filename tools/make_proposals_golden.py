"""tools/make_proposals_golden.py -- record tests/golden/proposals_golden.npz: what the reference's own get_proposals (data/ava.py:199-230)
makes of a short detector-proposal file.  Runs on the CPU, where the reference lies (STEP_REFERENCE, default /root/reference); only data
goes into the fixture -- the input text and the parsed result as arrays: video [R] (names), fid [R], box [R,4] float64, one row per kept
box in the dict's own order (videos, frames and boxes as first seen).  The text holds two videos, a score under 0.8 (dropped), a score of
exactly 0.8 (kept: the filter is `<`), a box repeated inside one frame (kept once), the same box in another frame (kept) and rows with
extra columns between the box and the score.  Modules data/ava.py imports that do not exist here (`cv2`, ...) are replaced by empty
stand-ins in `sys.modules` BEFORE the import, as tools/make_cls_golden.py does; get_proposals uses none of them.  The consumer is tests/proposal_cases.py (step_amd.selection.read_proposals)."""
import os
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("STEP_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "proposals_golden.npz")

TEXT = "\n".join([
    "vidA,0902,0.10,0.20,0.30,0.40,0.95",
    "vidA,0902,0.50,0.25,0.75,0.90,0.80",                    # exactly 0.8: kept
    "vidA,0902,0.10,0.20,0.30,0.40,0.99",                    # the first box again: kept once
    "vidA,0902,0.60,0.10,0.70,0.20,0.79",                    # under 0.8: dropped
    "vidA,0903,0.10,0.20,0.30,0.40,0.91",                    # the same box in another frame: kept
    "vidB,1000,0.05,0.05,0.55,0.95,12,3,0.85",               # extra columns: the score is the last one
    "vidB,1000,0.100,0.2,0.3,0.4,80,7,0.999",
    "vidB,0950,0.30,0.30,0.60,0.60,0.81",                    # frames in file order, not sorted
    "vidA,0902,0.11,0.20,0.30,0.40,1,2,0.9",
    "vidB,1000,0.05,0.05,0.55,0.95,0.92",                    # a repeat with another number of columns
]) + "\n"


class _StandIn(types.ModuleType):
    """an empty module whose every attribute is another one"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sub = _StandIn(self.__name__ + "." + name)
        setattr(self, name, sub)
        return sub


def import_reference():
    sys.path.insert(0, REF)
    for _ in range(16):
        try:
            import data.ava as M                                            # reference
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
    raise SystemExit("the reference's data.ava does not import")


def main():
    get_proposals = import_reference().get_proposals
    with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as f:
        f.write(TEXT)
    try:
        res = get_proposals(f.name)
    finally:
        os.unlink(f.name)
    video, fid, box = [], [], []
    for v, frames in res.items():
        for k, boxes in frames.items():
            for b in boxes:
                video.append(v)
                fid.append(k)
                box.append(b)
    np.savez(OUT, text=np.array(TEXT), video=np.array(video), fid=np.array(fid, np.int64), box=np.array(box, np.float64).reshape(-1, 4))
    print("wrote %s: %d rows kept of %d lines" % (OUT, len(fid), len(TEXT.splitlines())))


if __name__ == "__main__":
    main()
