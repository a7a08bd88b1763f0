"""Gradient-norm clipping and the device learning-rate schedules on the HOST interpreter build of the kernels (tests/emul): the C ABI
cases through tests.backends.EmuBackend, the optimizer / scheduler cases through the test-only interpreter patch.  The SAME cases run on
the real gfx950 library in tests/test_gpu_clip.py."""
import pytest

from tests import clip_cases as CC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", CC.KERNEL_CASES)
def test_emul_clip_kernel(name, bk, golden):
    getattr(CC, name)(bk, golden)


@pytest.mark.parametrize("name", CC.MODULE_CASES)
def test_emul_clip_module(name, golden):
    with emulated_kernels():
        getattr(CC, name)("cpu", golden)
