"""The reference's import path of the evaluation code; the implementation is mask_bev_amd/kitti_eval.py (K25 - K27)."""
