"""The reference's import path of the SemanticKITTI augmentations; the implementation is mask_bev_amd/augment.py (K23)."""
from mask_bev_amd.augment import make_augmentation, make_semantic_kitti_augmentation_list  # noqa: F401

__all__ = ['make_augmentation', 'make_semantic_kitti_augmentation_list']
