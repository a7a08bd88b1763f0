"""tools/make_lr_golden.py -- record tests/golden/lr_schedule_golden.json: the learning rates the reference's own WarmupCosineLR /
WarmupStepLR (utils/solver.py:96-172) leave in `param_groups`, iteration by iteration, as Python floats.  Runs on the CPU, where the
reference lies (STEP_REFERENCE, default /root/reference); only recorded numbers go into the fixture -- constructor arguments, base lrs
and, per case, lrs[k][i] = param_groups[i]['lr'] with last_epoch == first_epoch + k (k = 0 is what the constructor's own step leaves).
The consumers are tests/clip_cases.py (step_lr_schedule and the Device* schedulers of step_amd.optim)."""
import json
import os
import sys

import torch

REF = os.environ.get("STEP_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "lr_schedule_golden.json")
BASE_LRS = [1e-5, 5e-5, 1e-4]

CASES = [
    dict(name="cosine", kind="cosine", iters=120, last_epoch=-1,
         args=dict(milestones=[30, 60, 100], min_ratio=0.01, cycle_decay=0.5, warmup_iters=10, warmup_factor=0.1)),
    dict(name="cosine_plain", kind="cosine", iters=120, last_epoch=-1,
         args=dict(milestones=[30, 60, 100], min_ratio=0.0, cycle_decay=1.0, warmup_iters=10, warmup_factor=0.1)),
    dict(name="step", kind="step", iters=70, last_epoch=-1, args=dict(milestones=[30, 60], gamma=0.1, warmup_iters=10, warmup_factor=0.1)),
    dict(name="cosine_resumed", kind="cosine", iters=74, last_epoch=45,
         args=dict(milestones=[30, 60, 100], min_ratio=0.01, cycle_decay=0.5, warmup_iters=10, warmup_factor=0.1)),
]


def main():
    sys.path.insert(0, REF)
    from utils.solver import WarmupCosineLR, WarmupStepLR
    out = {"base_lrs": BASE_LRS, "cases": []}
    for case in CASES:
        params = [torch.nn.Parameter(torch.zeros(1)) for _ in BASE_LRS]
        groups = [{"params": [p], "lr": lr} for p, lr in zip(params, BASE_LRS)]
        if case["last_epoch"] != -1:
            for g in groups:
                g["initial_lr"] = g["lr"]
        opt = torch.optim.SGD(groups, lr=1e-3)
        cls = WarmupCosineLR if case["kind"] == "cosine" else WarmupStepLR
        sch = cls(opt, last_epoch=case["last_epoch"], **case["args"])
        first = sch.last_epoch
        lrs = []
        for k in range(case["iters"]):
            assert sch.last_epoch == first + k
            lrs.append([float(g["lr"]) for g in opt.param_groups])
            opt.step()
            sch.step()
        out["cases"].append(dict(name=case["name"], kind=case["kind"], args=case["args"], last_epoch=case["last_epoch"], first_epoch=first, lrs=lrs))
    a, b = out["cases"][0], out["cases"][3]
    assert b["first_epoch"] == 46 and b["lrs"] == a["lrs"][46:]          # the resumed run continues the uninterrupted one
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote %s: %s" % (OUT, [(c["name"], len(c["lrs"])) for c in out["cases"]]))


if __name__ == "__main__":
    main()
