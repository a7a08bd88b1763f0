"""Detector proposals on the device path, on the HOST interpreter build of the kernels (tests/emul): the C ABI cases of
tests/proposal_cases.py through tests.backends.EmuBackend, the module cases through the test-only interpreter patch, and the host case.
The SAME cases run on the real gfx950 library in tests/test_gpu_proposals.py."""
import gc
import os

import pytest

from tests import proposal_cases as RC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.fixture(scope="module", autouse=True)
def _small_footprint():
    """The suite runs in ONE process and the full-size oracle tests come later, so this module leaves nothing resident.  The interpreter
    starts a pool of threads per launch (HIPEMU_THREADS, read at every launch) and a worker's fiber stacks are not given back when it
    exits; the launches here have two or three workgroups, so they run on the calling thread, whose stacks are reused.  The restated
    states this module added to augplan_cases' session cache are dropped at the end."""
    saved = os.environ.get("HIPEMU_THREADS")
    os.environ["HIPEMU_THREADS"] = "1"
    yield
    if saved is None:
        del os.environ["HIPEMU_THREADS"]
    else:
        os.environ["HIPEMU_THREADS"] = saved
    RC.release()
    gc.collect()


@pytest.mark.parametrize("name", RC.KERNEL_CASES)
def test_emul_proposals_kernel(name, bk):
    RC.run_kernel_case(name, bk)


def test_read_proposals(tmp_path):
    RC.case_read_proposals(tmp_path)


@pytest.mark.parametrize("name", RC.MODULE_CASES)
def test_emul_proposals_module(name):
    with emulated_kernels():
        getattr(RC, name)("cpu")
