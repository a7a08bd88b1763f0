"""The device-side clip augmentation on the HOST interpreter build of the kernels (tests/emul): the host-only pins (plan parity with the
reference's RNG order, the numpy restatement against the fixture), the C ABI cases through tests.backends.EmuBackend and
step_amd.augment through the test-only interpreter patch.  The SAME cases run on the real gfx950 library in tests/test_gpu_augment.py."""
import pytest

from tests import augment_cases as AC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_plan_draws_the_reference_decisions_bit_for_bit(golden):
    AC.check_plan_parity(golden)


def test_numpy_restatement_of_the_pixel_pipeline_matches_the_fixture(golden):
    AC.check_numpy_restatement(golden)


def test_classes_are_exported():
    import step_amd

    assert step_amd.TubeAugmentation is AC.TubeAugmentation and step_amd.BaseTransform is AC.BaseTransform


@pytest.mark.parametrize("name", AC.KERNEL_CASES)
def test_emul_augment_kernel(name, bk, golden):
    getattr(AC, name)(bk, golden)


@pytest.mark.parametrize("name", AC.MODULE_CASES)
def test_emul_augment_module(name, golden):
    with emulated_kernels():
        getattr(AC, name)("cpu", golden)
