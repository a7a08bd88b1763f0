"""The classification pre-training stage on the HOST interpreter build of the kernels (tests/emul): the C ABI cases of tests/cls_cases.py
through tests.backends.EmuBackend, the module cases through the test-only interpreter patch, and the cases that need no kernel at all.  The
SAME cases run on the real gfx950 library in tests/test_gpu_cls.py."""
import pytest

from tests import cls_cases as CC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", CC.KERNEL_CASES)
def test_emul_cls_kernel(name, bk, golden):
    getattr(CC, name)(bk, golden)


@pytest.mark.parametrize("name", CC.HOST_CASES)
def test_cls_host(name, golden):
    getattr(CC, name)(golden)


@pytest.mark.parametrize("name", CC.MODULE_CASES)
def test_emul_cls_module(name, golden):
    with emulated_kernels():
        getattr(CC, name)("cpu", golden)
