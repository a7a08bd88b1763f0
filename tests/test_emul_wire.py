"""The bf16 gradient wire on the HOST interpreter build of the kernels (tests/emul): the C ABI cases through tests.backends.EmuBackend, the
GradWire / BucketedReducer / allreduce_flat cases through the test-only interpreter patch, on host tensors in a one-rank gloo group.  The
SAME cases run on the real gfx950 library in tests/test_gpu_wire.py."""
import pytest

from tests import wire_cases as WC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("name", WC.KERNEL_CASES)
def test_emul_wire_kernel(name, bk, golden):
    getattr(WC, name)(bk, golden)


@pytest.mark.parametrize("name", WC.MODULE_CASES)
def test_emul_wire_module(name, golden):
    with emulated_kernels():
        getattr(WC, name)("cpu", golden)
