"""The pixel-split form of step_conv_forward_group's narrow members on the real gfx950 library: the cases of tests/narrow_cases.py
(shared with the interpreter run of tests/test_emul_narrow.py) plus C2's own 28x28 members under the default option value."""
import pytest

from tests import narrow_cases as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", NC.KERNEL_CASES + NC.KERNEL_GPU_ONLY)
def test_gpu_narrow(name, bk, golden):
    getattr(NC, name)(bk, golden)
