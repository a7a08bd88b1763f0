"""The device-drawn clip augmentation on the HOST interpreter build of the kernels (tests/emul): the C ABI cases of tests/augplan_cases.py
through tests.backends.EmuBackend, the module cases through the test-only interpreter patch, and the cases that need no kernel at all.  The
SAME cases run on the real gfx950 library in tests/test_gpu_augplan.py."""
import pytest

from tests import augplan_cases as PC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", PC.KERNEL_CASES)
def test_emul_augplan_kernel(name, bk):
    PC.run_kernel_case(name, bk)


@pytest.mark.parametrize("name", PC.HOST_CASES)
def test_augplan_host(name):
    getattr(PC, name)()


@pytest.mark.parametrize("name", PC.MODULE_CASES)
def test_emul_augplan_module(name):
    with emulated_kernels():
        getattr(PC, name)("cpu")
