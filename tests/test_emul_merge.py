"""The cross-class merge of detections on the HOST interpreter build of the kernels (tests/emul): the C ABI cases through
tests.backends.EmuBackend, driver.postprocess_merged / merged_csv through the test-only interpreter patch, and the host-side pin of the
fixture (no kernel at all).  The SAME cases run on the real gfx950 library in tests/test_gpu_merge.py."""
import pytest

from tests import merge_cases as MG
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_numpy_restatement_of_the_merge_matches_the_fixture(golden):
    MG.check_numpy_restatement(golden)


@pytest.mark.parametrize("name", MG.KERNEL_CASES)
def test_emul_merge_kernel(name, bk, golden):
    getattr(MG, name)(bk, golden)


@pytest.mark.parametrize("name", MG.MODULE_CASES)
def test_emul_merge_module(name, golden):
    with emulated_kernels():
        getattr(MG, name)("cpu", golden)
