"""The frame-mAP evaluation on the HOST interpreter build of the kernels (tests/emul): the C ABI cases through tests.backends.EmuBackend,
step_amd.evaluate.FrameMAP through the test-only interpreter patch, and the host-side pin of the fixture (no kernel at all).  The SAME
cases run on the real gfx950 library in tests/test_gpu_eval.py."""
import pytest

from tests import eval_cases as EV
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_numpy_restatement_of_the_evaluation_matches_the_fixture(golden):
    EV.check_numpy_restatement(golden)


@pytest.mark.parametrize("name", EV.KERNEL_CASES)
def test_emul_eval_kernel(name, bk, golden):
    getattr(EV, name)(bk, golden)


@pytest.mark.parametrize("name", EV.MODULE_CASES)
def test_emul_eval_module(name, golden):
    with emulated_kernels():
        getattr(EV, name)("cpu", golden)
