"""Tube growth outside temporal_mode "predict" on the HOST interpreter build of the kernels (tests/emul): the C ABI cases of
tests/tubemode_cases.py through tests.backends.EmuBackend, the DeviceSelector cases through the test-only interpreter patch.  The SAME cases
run on the real gfx950 library in tests/test_gpu_tubemode.py."""
import pytest

from tests import tubemode_cases as TC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", TC.KERNEL_CASES)
def test_emul_tubemode_kernel(name, bk, golden):
    getattr(TC, name)(bk, golden)


@pytest.mark.parametrize("name", TC.MODULE_CASES)
def test_emul_tubemode_module(name, golden):
    with emulated_kernels():
        getattr(TC, name)("cpu", golden)
