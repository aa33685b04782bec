"""Same public names as the reference's ``layers`` package (layers/__init__.py:1-2, functions/__init__.py:1-9,
modules/__init__.py:1-12) for the components on the hot path."""
from .box_utils import center_size, crop, decode, encode, jaccard, mask_iou, match, match_batch, point_form, \
    sanitize_coordinates, sanitize_coordinates_hw  # noqa: F401
from .conf_loss import ohem_conf_loss, select_neg_bboxes  # noqa: F401
from .functions import CandidateShift, Detect, Detect_TF, Track, Track_TF, compute_comp_scores, generate_candidate, \
    merge_candidates  # noqa: F401
from .mask_utils import generate_mask, generate_mask_rows, lincomb_mask_loss_image, mask_bce_sum  # noqa: F401
from .pos_loss import box_center_loss, track_loss  # noqa: F401
from .t2s_loss import track_to_segment_loss  # noqa: F401
from .multibox_loss import MultiBoxLoss, lincomb_mask_loss  # noqa: F401
from .modules import FPN, FeatureAlign, InterpolateModule, PredictionModule_FC, TemporalNet, bbox_feat_extractor, \
    correlate, make_net  # noqa: F401
from .t2s_feat import t2s_concat_feat  # noqa: F401
