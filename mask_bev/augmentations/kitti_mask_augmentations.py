"""The reference's import path of the KITTI augmentations; the implementation is mask_bev_amd/augment.py (K23) and, for
``BoxNoise`` (``object_noise``) and ``ObjectSample``, mask_bev_amd/object_augment.py (K28)."""
from mask_bev_amd.augment import _KITTI_CONSTRUCTORS, make_kitti_augmentation_list  # noqa: F401
from mask_bev_amd.augment import make_augmentation as _make_augmentation
from mask_bev_amd.object_augment import ObjectNoise as BoxNoise, ObjectSample  # noqa: F401


def make_augmentation(args):
    return _make_augmentation(args, _KITTI_CONSTRUCTORS)


__all__ = ['make_augmentation', 'make_kitti_augmentation_list', 'BoxNoise', 'ObjectSample']
