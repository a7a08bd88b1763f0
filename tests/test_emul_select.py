"""The device-side proposal selection on the HOST interpreter build of the kernels (tests/emul): the C ABI cases through
tests.backends.EmuBackend, the DeviceSelector cases through the test-only interpreter patch.  The SAME cases run on the real gfx950
library in tests/test_gpu_select.py."""
import pytest

from tests import select_cases as SC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", SC.KERNEL_CASES)
def test_emul_select_kernel(name, bk, golden):
    getattr(SC, name)(bk, golden)


@pytest.mark.parametrize("name", SC.MODULE_CASES)
def test_emul_select_module(name, golden):
    with emulated_kernels():
        getattr(SC, name)("cpu", golden)
