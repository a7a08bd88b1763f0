"""step_amd -- MI355X (gfx950) implementation of the STEP hot path: I3D backbone, two-branch head,
ROIAlign / ROIPool / NMS.  Drop-in for the reference's `models` package and
`external.maskrcnn_benchmark.roi_layers` package."""
from .backbone import BaseNet, I3D, I3D_head, build_base_i3d, weights_init  # noqa: F401
from .heads import ContextNet, Dropout, ROINet, TwoBranchNet  # noqa: F401
from . import rng  # noqa: F401
from .rng import DeviceRNG, manual_seed  # noqa: F401
from . import dist  # noqa: F401
from .optim import DeviceWarmupCosineLR, DeviceWarmupStepLR, FlatAdam, FlatSGD, LossScaler  # noqa: F401
from . import evaluate  # noqa: F401
from .evaluate import FrameMAP, ava_evaluation  # noqa: F401
from . import augment  # noqa: F401
from .augment import BaseTransform, DeviceTubeAugmentation, TubeAugmentation  # noqa: F401
from . import video  # noqa: F401
from .video import FrameRing, VideoClips, clip_frame_indices, detect_video  # noqa: F401

__all__ = ["BaseNet", "ROINet", "TwoBranchNet", "ContextNet", "I3D", "I3D_head", "FrameMAP", "ava_evaluation",
           "TubeAugmentation", "DeviceTubeAugmentation", "BaseTransform", "Dropout", "DeviceRNG", "manual_seed", "FrameRing", "VideoClips", "clip_frame_indices",
           "detect_video"]
__version__ = "0.1.0"
