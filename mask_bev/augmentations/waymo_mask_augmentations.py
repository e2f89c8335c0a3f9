"""The reference's import path of the Waymo augmentations; the implementation is mask_bev_amd/augment.py (K23)."""
from mask_bev_amd.augment import _WAYMO_CONSTRUCTORS, make_waymo_augmentation_list  # noqa: F401
from mask_bev_amd.augment import make_augmentation as _make_augmentation


def make_augmentation(aug):
    return _make_augmentation(aug, _WAYMO_CONSTRUCTORS, rand_augment=False)


__all__ = ['make_augmentation', 'make_waymo_augmentation_list']
