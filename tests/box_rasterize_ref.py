"""The fill rule of K24 (csrc/box_rasterize.hip) in plain numpy integers: the oracle of the box-rasteriser tests.  The
product never imports this file.

Input per box: four integer vertices v0..v3 in cell coordinates (px, py) — the reference's box corners after ``_map_to``
and ``np.intp`` (kitti_rasterizer.py:49-52, waymo_rasterizer.py:39-42; truncation toward zero).  A cell (px, py) belongs
to the box iff it is in I ∪ L:

  I  the integer point lies inside or on the closed quadrilateral v0 v1 v2 v3: it lies on an edge (cross product 0 and
     inside the edge's bounding box), or a ray towards +x crosses an odd number of edges.  An edge a → b is crossed iff
     (ay > py) != (by > py) and the sign of the cross product (bx - ax)(py - ay) - (by - ay)(px - ax) says the crossing
     lies to the right: > 0 for by > ay, < 0 for by < ay.  Exact integers (the kernel's products are 64-bit); the vertex
     order may run either way; a quadrilateral that truncation folded is filled even-odd.
  L  the point lies on the line between two consecutive vertices (v3 → v0 included): with dx = bx - ax, dy = by - ay,
     n = max(|dx|, |dy|), the points (ax + floor((2 i dx + n) / (2 n)), ay + floor((2 i dy + n) / (2 n))), i = 0 .. n
     (n = 0: the single point).  Along the major axis that is one cell per step; on the minor axis a tie rounds up.

Cells outside the grid are dropped.  Boxes are painted in table order, a later box overwrites an earlier one
(the reference's loop).  Equality with ``cv2.drawContours(mask, [contour], 0, 255, -1)`` is NOT pinned by any test: OpenCV
draws the outline with its own line iterator and fills spans in 16-bit fixed point, so tie cells on an edge may differ;
for a 4 m x 1.8 m box on 0.1 - 0.16 m cells that can only touch boundary cells of a mask.
"""
import numpy as np


def line_cells(a, b) -> np.ndarray:
    """(n + 1, 2) int64 cells of the line a → b."""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    dx, dy = bx - ax, by - ay
    n = max(abs(dx), abs(dy))
    if n == 0:
        return np.array([[ax, ay]], dtype=np.int64)
    i = np.arange(n + 1, dtype=np.int64)
    return np.stack([ax + (2 * i * dx + n) // (2 * n), ay + (2 * i * dy + n) // (2 * n)], axis=1)


def inside_closed(verts, px: np.ndarray, py: np.ndarray) -> np.ndarray:
    """The set I for integer arrays px, py (broadcast together) → bool array."""
    px, py = np.asarray(px, dtype=np.int64), np.asarray(py, dtype=np.int64)
    on = np.zeros(np.broadcast(px, py).shape, dtype=bool)
    odd = np.zeros_like(on)
    for e in range(4):
        ax, ay = int(verts[e][0]), int(verts[e][1])
        bx, by = int(verts[(e + 1) % 4][0]), int(verts[(e + 1) % 4][1])
        dx, dy = bx - ax, by - ay
        cross = dx * (py - ay) - dy * (px - ax)
        on |= (cross == 0) & (px >= min(ax, bx)) & (px <= max(ax, bx)) & (py >= min(ay, by)) & (py <= max(ay, by))
        straddles = (ay > py) != (by > py)
        odd ^= straddles & ((cross > 0) if dy > 0 else (cross < 0))
    return on | odd


def box_cells(verts, nx: int, ny: int) -> np.ndarray:
    """(nx, ny) bool: the cells of one box, I ∪ L, clipped to the grid."""
    verts = np.asarray(verts, dtype=np.int64).reshape(4, 2)
    out = np.zeros((nx, ny), dtype=bool)
    x0, x1 = max(int(verts[:, 0].min()), 0), min(int(verts[:, 0].max()), nx - 1)
    y0, y1 = max(int(verts[:, 1].min()), 0), min(int(verts[:, 1].max()), ny - 1)
    if x0 <= x1 and y0 <= y1:                      # I and L both lie inside the vertices' bounding box
        gx, gy = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1), indexing='ij')
        out[x0:x1 + 1, y0:y1 + 1] = inside_closed(verts, gx, gy)
    for e in range(4):
        c = line_cells(verts[e], verts[(e + 1) % 4])
        c = c[(c[:, 0] >= 0) & (c[:, 0] < nx) & (c[:, 1] >= 0) & (c[:, 1] < ny)]
        out[c[:, 0], c[:, 1]] = True
    return out


def rasterize_boxes(vertices, ids, nx: int, ny: int) -> np.ndarray:
    """vertices (n, 4, 2) int, ids (n) int → (nx, ny) int32 map: map[px, py] = the id of the last box holding the cell."""
    vertices = np.asarray(vertices, dtype=np.int64).reshape(-1, 4, 2)
    m = np.zeros((nx, ny), dtype=np.int32)
    for v, i in zip(vertices, np.asarray(ids).reshape(-1)):
        m[box_cells(v, nx, ny)] = int(i)
    return m


def rasterize_batch(vertices, ids, frame_offsets, nx: int, ny: int) -> np.ndarray:
    """The whole call of ``mbv_rasterize_boxes``: (B, nx, ny) int32."""
    vertices, ids = np.asarray(vertices).reshape(-1, 4, 2), np.asarray(ids).reshape(-1)
    return np.stack([rasterize_boxes(vertices[a:b], ids[a:b], nx, ny)
                     for a, b in zip(frame_offsets[:-1], frame_offsets[1:])])


def draw_contours_fill(mask: np.ndarray, contours, contour_idx, color, thickness) -> np.ndarray:
    """Stand-in for ``cv2.drawContours(mask, [contour], 0, color, -1)`` on a (rows, cols) image: a contour point is (x, y) =
    (column, row).  Used by tests/golden/make_golden_boxes.py; it is the fill above, not OpenCV's."""
    assert thickness == -1 and contour_idx == 0 and len(contours) == 1
    rows, cols = mask.shape
    cells = box_cells(np.asarray(contours[0]).reshape(4, 2), cols, rows)          # [x][y]
    mask[cells.T] = color
    return mask
