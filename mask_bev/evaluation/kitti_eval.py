"""The reference's import path of the KITTI evaluation; the implementation is mask_bev_amd/kitti_eval.py (BEV and 3D
metrics on the device: K25 boxes, K31 heights, K26 / K26b overlaps, K27 statistics)."""
from mask_bev_amd.kitti_eval import (bev_box_overlap, clean_data, d3_box_overlap, eval_class, eval_kitti, get_mAP,  # noqa: F401
                                     get_mAP_v2, get_official_eval_result, get_thresholds, mask_to_pred)

__all__ = ['bev_box_overlap', 'clean_data', 'd3_box_overlap', 'eval_class', 'eval_kitti', 'get_mAP', 'get_mAP_v2',
           'get_official_eval_result', 'get_thresholds', 'mask_to_pred']
