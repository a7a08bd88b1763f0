"""tools/make_ops_profile_golden.py -- writes tests/golden/ops_profile_records.json: what every instrumented wrapper of step_amd.ops
appends to ops.PROFILE -- (kernel name, algorithmic FLOPs, algorithmic bytes), the inputs of bench.py's roofline -- for the calls of
tests.module_cases.ops_profile_calls, on the interpreter build of the library (tests/emul) with nothing launched (PROFILE_LIMIT = 0).

The call list lives with the case that reads the fixture (tests.module_cases.case_ops_profile_records).  Regenerate only on purpose --
a new wrapper in the list, a kernel renamed, a planner rule changed -- and from a commit whose records are known to be right: the
fixture exists to hold them still while step_amd/ops.py is rewritten.

    python tools/make_ops_profile_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import module_cases as MC  # noqa: E402
from tests.emul.patch import emulated_kernels  # noqa: E402


def main():
    with emulated_kernels():
        rec = MC.ops_profile_records("cpu")
    for tag, rows in rec.items():
        assert rows, "%s recorded nothing: the wrapper returned None -- a wrong shape" % tag
        for name, flops, nbytes in rows:
            print("%-36s %-110s %14.0f %12.0f" % (tag, name[:110], flops, nbytes))
    path = os.path.join(MC.GOLDEN, "ops_profile_records.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("%s: %d calls, %d records, %d bytes" % (os.path.basename(path), len(rec), sum(len(r) for r in rec.values()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
