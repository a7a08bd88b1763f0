"""The pixel-split form of step_conv_forward_group's narrow members on the HOST interpreter build of the kernels (tests/emul): the
cases of tests/narrow_cases.py through tests.backends.EmuBackend.  The SAME cases run on the real gfx950 library in
tests/test_gpu_narrow.py."""
import pytest

from tests import narrow_cases as NC
from tests.backends import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", NC.KERNEL_CASES)
def test_emul_narrow(name, bk, golden):
    getattr(NC, name)(bk, golden)
