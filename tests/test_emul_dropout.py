"""The device-side dropout on the HOST interpreter build of the kernels (tests/emul): the C ABI cases through
tests.backends.EmuBackend, the Dropout / DeviceRNG / TwoBranchNet cases through the test-only interpreter patch.  The SAME cases run
on the real gfx950 library in tests/test_gpu_dropout.py."""
import pytest

from tests import dropout_cases as DC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", DC.KERNEL_CASES)
def test_emul_dropout_kernel(name, bk, golden):
    getattr(DC, name)(bk, golden)


@pytest.mark.parametrize("name", DC.MODULE_CASES)
def test_emul_dropout_module(name, golden):
    with emulated_kernels():
        getattr(DC, name)("cpu", golden)
