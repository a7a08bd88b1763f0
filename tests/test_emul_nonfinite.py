"""NaN / inf conformance of the forward kernels on the HOST interpreter build (tests/emul): the cases of tests/nonfinite_cases.py through
tests.backends.EmuBackend and, for the module cases the interpreter can run in reasonable time, through the test-only interpreter
patch.  The SAME cases run on the real gfx950 library in tests/test_gpu_nonfinite.py."""
import pytest

from tests import nonfinite_cases as NF
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", NF.KERNEL_CASES)
def test_emul_nonfinite_kernel(name, bk, golden):
    getattr(NF, name)(bk, golden)


@pytest.mark.parametrize("name", NF.CPU_MODULE_CASES)
def test_emul_nonfinite_module(name, golden):
    with emulated_kernels():
        getattr(NF, name)("cpu", golden)
