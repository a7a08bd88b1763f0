"""NaN / inf conformance of the forward kernels on the real gfx950 library: the cases of tests/nonfinite_cases.py (shared with the
interpreter run of tests/test_emul_nonfinite.py).  The device build stages operands and takes its maxima differently from the
interpreter build (LDS-DMA, packed 16-bit integer keys, v_pk_maximum3_f16, the matrix unit's own NaN), so it is checked here."""
import pytest

from tests import nonfinite_cases as NF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    from tests.backends import GpuBackend

    return GpuBackend()


@pytest.mark.parametrize("name", NF.KERNEL_CASES)
def test_gpu_nonfinite_kernel(name, bk, golden):
    getattr(NF, name)(bk, golden)


@pytest.mark.parametrize("name", NF.MODULE_CASES)
def test_gpu_nonfinite_module(name, golden):
    getattr(NF, name)("cuda", golden)
