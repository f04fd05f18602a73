"""MI355X-native frame-importance scorer (drop-in for the reference ``model.SimNet``).

The directory name carries a hyphen, so import it with
``importlib.import_module("video-summarization_amd")`` or through the root-level alias
module ``video_summarization_amd``.
"""
from . import _lib, synth  # noqa: F401
from .simnet import SimNet, score_frames  # noqa: F401
from .pretrain import PretrainModel  # noqa: F401
from .losses import mse_packed_loss, mse_with_mask_loss  # noqa: F401
from . import segmentation  # noqa: F401
from . import optim  # noqa: F401
from .optim import Adam, AdamW, clip_grad_norm_, grad_norm  # noqa: F401
from .data import PretrainSet, TrainSet, collate_fn_pretrain_packed, epoch_plan  # noqa: F401
from .harness import pretrain_epoch_resident, pretrain_step_packed, train_epoch_resident  # noqa: F401
from .segmentation import get_segment_fn, kts_seg, kts_seg_batch  # noqa: F401
from . import summary  # noqa: F401
from .summary import summarize, summarize_scores  # noqa: F401
from . import features  # noqa: F401
from .features import GoogLeNetFeatures, get_google_net_features, resize_frames_device, resize_output_size  # noqa: F401
from . import video_features  # noqa: F401
from .video_features import R3D18Features, get_video_feature  # noqa: F401

__all__ = ["SimNet", "PretrainModel", "score_frames", "synth", "mse_with_mask_loss", "mse_packed_loss", "segmentation", "get_segment_fn", "kts_seg",
           "kts_seg_batch", "optim", "Adam", "AdamW", "clip_grad_norm_", "grad_norm", "collate_fn_pretrain_packed", "pretrain_step_packed", "summary", "summarize",
           "summarize_scores", "TrainSet", "PretrainSet", "epoch_plan", "train_epoch_resident", "pretrain_epoch_resident", "features",
           "GoogLeNetFeatures", "get_google_net_features", "resize_frames_device", "resize_output_size", "video_features", "R3D18Features",
           "get_video_feature"]
