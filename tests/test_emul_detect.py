"""The fused detection tail for clips of more than 64 tubes on the HOST interpreter build of the kernels (tests/emul): the C ABI cases
through tests.backends.EmuBackend, driver.postprocess / postprocess_merged / classified_rows through the test-only interpreter patch, and
the host-side pin of the fixture (no kernel at all).  The SAME cases run on the real gfx950 library in tests/test_gpu_detect.py."""
import pytest

from tests import detect_cases as DC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_detect_block_fixture_holds_groups_past_a_wavefront(golden):
    DC.check_fixture(golden)


@pytest.mark.parametrize("name", DC.KERNEL_CASES)
def test_emul_detect_kernel(name, bk, golden):
    getattr(DC, name)(bk, golden)


@pytest.mark.parametrize("name", DC.MODULE_CASES)
def test_emul_detect_module(name, golden):
    with emulated_kernels():
        getattr(DC, name)("cpu", golden)
