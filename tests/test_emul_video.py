"""The video demo's input side on the HOST interpreter build of the kernels (tests/emul): index parity with the reference's loader, the
C ABI cases of step_clip_gather_u8 through tests.backends.EmuBackend, and step_amd.video (FrameRing, VideoClips) through the test-only
interpreter patch.  The SAME cases run on the real gfx950 library in tests/test_gpu_video.py."""
import pytest

from tests import video_cases as VC
from tests.backends import EmuBackend
from tests.emul.patch import emulated_kernels


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


def test_clip_frame_indices_match_the_reference_loader():
    VC.check_index_parity()


def test_video_names_are_exported():
    import step_amd

    assert step_amd.FrameRing is VC.FrameRing and step_amd.VideoClips is VC.VideoClips
    assert step_amd.clip_frame_indices is VC.clip_frame_indices and callable(step_amd.detect_video)


@pytest.mark.parametrize("name", VC.KERNEL_CASES)
def test_emul_video_kernel(name, bk):
    with emulated_kernels():
        getattr(VC, name)(bk, "cpu")


@pytest.mark.parametrize("name", VC.MODULE_CASES)
def test_emul_video_module(name, bk):
    with emulated_kernels():
        getattr(VC, name)(bk, "cpu")
