"""The reference's import path of the KITTI evaluation; the implementation is mask_bev_amd/kitti_eval.py (BEV metric on
the device: K25 boxes, K26 overlaps, K27 statistics)."""
from mask_bev_amd.kitti_eval import (bev_box_overlap, clean_data, eval_class, eval_kitti, get_mAP, get_mAP_v2,  # noqa: F401
                                     get_official_eval_result, get_thresholds, mask_to_pred)

__all__ = ['bev_box_overlap', 'clean_data', 'eval_class', 'eval_kitti', 'get_mAP', 'get_mAP_v2', 'get_official_eval_result',
           'get_thresholds', 'mask_to_pred']
