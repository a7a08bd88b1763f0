"""step_pool_then_conv_forward on the real gfx950 library: the cases of tests/poolpw_cases.py (shared with the interpreter run of
tests/test_emul_poolpw.py) plus C2's own 28x28 layers under the default option value."""
import pytest

from tests import poolpw_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", PC.KERNEL_CASES + PC.KERNEL_GPU_ONLY)
def test_gpu_poolpw(name, bk, golden):
    getattr(PC, name)(bk, golden)
