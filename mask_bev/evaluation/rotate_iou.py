"""The reference's import path of the rotated-box IoU; the kernel is K26 (mask_bev_amd/csrc/rotate_iou.hip).  The angle
turns counter-clockwise, as in ``mask_bev_amd.rasterize.box_vertices`` (the reference's numba kernel turns clockwise)."""
import numpy as np

from mask_bev_amd.kitti_eval import bev_box_overlap


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """boxes (N, 5), query_boxes (K, 5) arrays [x, y, dx, dy, angle] → (N, K) overlaps in the dtype of ``boxes``."""
    boxes = np.asarray(boxes)
    out = bev_box_overlap(boxes, query_boxes, criterion, device=f'cuda:{device_id}')
    return out.astype(boxes.dtype if boxes.dtype.kind == 'f' else np.float32)


__all__ = ['rotate_iou_gpu_eval']
