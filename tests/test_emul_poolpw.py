"""step_pool_then_conv_forward (pool + pointwise conv in one launch, no pooled tensor) on the HOST interpreter build of the kernels
(tests/emul): the cases of tests/poolpw_cases.py through tests.backends.EmuBackend.  The SAME cases run on the real gfx950 library in
tests/test_gpu_poolpw.py."""
import pytest

from tests import poolpw_cases as PC
from tests.backends import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", PC.KERNEL_CASES)
def test_emul_poolpw(name, bk, golden):
    getattr(PC, name)(bk, golden)
