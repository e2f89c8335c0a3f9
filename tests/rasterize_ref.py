"""Plain numpy / scipy.ndimage restatement of the reference's SemanticKittiRasterizer.get_mask_around
(mask_bev/datasets/semantic_kitti/semantic_kitti_rasterizer.py:41-94) and SceneMaker.add_scan
(semantic_kitti_scene.py:54-61), used by the K22 tests only — the product never imports it.

The transform, the strict range test, the floor division, the instance selection and the composition follow the
reference line by line (tests/golden/rasterizer.npz pins them against the reference's own class).  The morphology is
restated from OpenCV's published behaviour: ``cv2.morphologyEx(MORPH_CLOSE / MORPH_OPEN)`` with a k x k MORPH_RECT
element, anchor at the centre, BORDER_CONSTANT with ``morphologyDefaultBorderValue`` — a cell outside the image never
wins: it counts as set for an erosion and as clear for a dilation.

The paint order is an argument: the reference iterates a Python set of numpy.uint32 (hash order); the default here is
ascending id, i.e. the highest id wins an overlap, which is K22's rule.
"""
import numpy as np
from scipy import ndimage


def grid_size(lo_hi, voxel_size) -> int:
    return int((lo_hi[1] - lo_hi[0]) / voxel_size)


def dilate(img: np.ndarray, k: int) -> np.ndarray:
    return ndimage.grey_dilation(img, size=(k, k), mode='constant', cval=0)


def erode(img: np.ndarray, k: int) -> np.ndarray:
    return ndimage.grey_erosion(img, size=(k, k), mode='constant', cval=255)


def close_open(occ: np.ndarray, k: int) -> np.ndarray:
    """(nx, ny) {0, 1} uint8 -> MORPH_CLOSE then MORPH_OPEN with the k x k square (:87-88)."""
    img = occ.astype(np.uint8)
    img = erode(dilate(img, k), k)
    img = dilate(erode(img, k), k)
    return img


def aggregate_scene(points, poses):
    """SceneMaker.add_scan: per-scan (n, >=3) points and (4, 4) velo-to-pose matrices -> (N, 4) f64 world-frame scene."""
    out = []
    for pc, tr in zip(points, poses):
        homo = np.zeros((pc.shape[0], 4))
        homo[:, :3] = pc[:, :3]
        homo[:, 3] = 1
        homo = (np.asarray(tr, dtype=np.float64) @ homo.T).T
        homo[:, :3] /= homo[:, 3].reshape((-1, 1))
        out.append(homo)
    return np.concatenate(out) if out else np.zeros((0, 4))


def cells_of(scene_pc, inst, inv_pose, x_range, y_range, z_range, voxel_size):
    """:53-68 — (kept instance labels, (n, 2) cell indices) of a world-frame scene seen from the centre scan."""
    homo = np.array(scene_pc, dtype=np.float64, copy=True)
    if homo.shape[1] == 3:
        homo = np.hstack([homo, np.ones((homo.shape[0], 1))])
    homo[:, 3] = 1
    homo = (np.asarray(inv_pose, dtype=np.float64) @ homo.T).T
    homo /= homo[:, 3].reshape((-1, 1))
    with np.errstate(invalid='ignore'):
        in_range = (x_range[0] < homo[:, 0]) & (homo[:, 0] < x_range[1]) & \
                   (y_range[0] < homo[:, 1]) & (homo[:, 1] < y_range[1]) & \
                   (z_range[0] < homo[:, 2]) & (homo[:, 2] < z_range[1])
    homo = homo[in_range]
    ix = np.floor((homo[:, 0] - x_range[0]) / voxel_size).astype(int)
    iy = np.floor((homo[:, 1] - y_range[0]) / voxel_size).astype(int)
    return np.asarray(inst)[in_range], np.stack([ix, iy]).T


def get_mask_around(scene_pc, scene_inst, inv_pose, x_range, y_range, z_range, voxel_size, centre_inst=None,
                    remove_unseen=False, min_points=1, morph_kernel_size=9, order=None, return_masks=False):
    """The instance map (nx, ny) int64 of a world-frame scene.  ``order``: the ids in paint order (later over earlier);
    None = ascending.  ``return_masks``: also a dict id -> closed-and-opened (nx, ny) bool mask."""
    nx, ny = grid_size(x_range, voxel_size), grid_size(y_range, voxel_size)
    inst, idx = cells_of(scene_pc, scene_inst, inv_pose, x_range, y_range, z_range, voxel_size)
    keep = (idx[:, 0] < nx) & (idx[:, 1] < ny) if idx.size else np.zeros((0,), dtype=bool)
    inst, idx = inst[keep], idx[keep]
    if remove_unseen:
        centre_inst = np.asarray(centre_inst)
        present = set(int(i) for i in np.unique(centre_inst) if i != 0
                      and np.count_nonzero(centre_inst == i) >= min_points)
    else:
        present = set(int(i) for i in np.unique(inst)) - {0}
    ids = sorted(present) if order is None else [int(i) for i in order]
    assert set(ids) == present, (sorted(ids), sorted(present))
    out = np.zeros((nx, ny), dtype=np.int64)
    masks = {}
    for i in ids:
        occ = np.zeros((nx, ny), dtype=np.uint8)
        sel = idx[inst == i]
        occ[sel[:, 0], sel[:, 1]] = 1
        m = close_open(occ, morph_kernel_size) > 0.5
        masks[i] = m
        out[m] = i
    return (out, masks) if return_masks else out


def paint_occupancies(occ, ids, k):
    """K22b alone: occ (S, nx, ny) {0, 1}, ids (S) ascending or not -> map with the highest id on top."""
    out = np.zeros(occ.shape[1:], dtype=np.int64)
    for s in np.argsort(np.asarray(ids), kind='stable'):
        out[close_open(occ[s], k) > 0] = int(ids[s])
    return out
