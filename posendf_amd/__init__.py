"""posendf_amd -- MI355X-native Pose-NDF distance / projection engine (gfx950 HIP kernels).

`from posendf_amd import PoseNDF` is the drop-in for `from model.posendf import PoseNDF` of the reference.
"""
from . import synth  # noqa: F401
from .config import amass_config, load_config  # noqa: F401


def __getattr__(name):   # torch is imported lazily so that numpy-only users (oracle, packer tests) stay light
    if name in ("PoseNDF", "gradient"):
        from . import facade
        return getattr(facade, name)
    if name == "PoseIndex":
        from .knn import PoseIndex
        return PoseIndex
    if name in ("Trainer", "PoseDataset"):
        from . import trainer
        return getattr(trainer, name)
    if name in ("OnlinePoseDataset", "OnlineOptions", "sample_noisy"):
        from . import online
        return getattr(online, name)
    if name == "PoseCompletion":
        from .pose_completion import PoseCompletion
        return PoseCompletion
    if name == "PoseInterpolation":
        from .pose_interpolation import PoseInterpolation
        return PoseInterpolation
    if name in ("PoseDenoising", "denoise_track_file"):
        from . import pose_denoising
        return getattr(pose_denoising, name)
    if name in ("KeypointFitting", "fit_keypoint_file", "view_tables"):
        from . import keypoint_fitting
        return getattr(keypoint_fitting, name)
    if name in ("SkeletonPoseNDF", "SKELETONS", "skeleton_config", "forward_kinematics", "camera_project", "view_table"):
        from . import skeleton
        return getattr(skeleton, name)
    if name == "BodyModel":
        from .body_model import BodyModel
        return BodyModel
    if name in ("ImageFit", "PerspectiveCamera", "keypoint_term"):
        from . import image_fitting
        return getattr(image_fitting, name)
    raise AttributeError(name)


__all__ = ["PoseNDF", "gradient", "BodyModel", "PoseIndex", "Trainer", "PoseDataset", "OnlinePoseDataset", "OnlineOptions", "sample_noisy", "ImageFit", "PerspectiveCamera", "keypoint_term", "PoseCompletion", "PoseInterpolation",
           "PoseDenoising", "denoise_track_file",
           "KeypointFitting", "fit_keypoint_file", "view_tables",
           "SkeletonPoseNDF", "SKELETONS", "skeleton_config", "forward_kinematics", "camera_project", "view_table",
           "amass_config", "load_config", "synth"]
