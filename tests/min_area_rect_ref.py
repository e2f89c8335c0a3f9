"""Plain restatement of K30a (largest 8-connected component of a mask) and K30b (minimum-area rectangle of a mask's set
cells), written from the words of include/maskbev_hip.h — the yardstick of tests/test_k30_min_area_rect_gpu.py.

Components come from ``scipy.ndimage.label`` with a 3 x 3 structure; its labels are numbered in raster order of each
component's first cell, so "the first of the largest" is the header's tie rule.  The hull is a monotone chain in Python
ints, areas are ``fractions.Fraction`` (exact), and only the box of the chosen direction is float64 (numpy)."""
from fractions import Fraction

import numpy as np
from scipy import ndimage


# ------------------------------------------------------------------------------------------------ K30a
def largest_component(mask):
    """mask (H, W) bool → (kept (H, W) bool, n, components): the 8-connected component with the most cells; among equals the
    one holding the lowest raster index."""
    mask = np.asarray(mask, dtype=bool)
    labels, count = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))
    if count == 0:
        return np.zeros_like(mask), 0, 0
    sizes = np.bincount(labels.reshape(-1), minlength=count + 1)[1:]
    first = ndimage.minimum(np.arange(mask.size).reshape(mask.shape), labels, np.arange(1, count + 1))
    assert np.all(np.diff(first) > 0)                                  # labels are in raster order of the first cell
    best = int(np.argmax(sizes))                                       # argmax: the first of the largest
    return labels == best + 1, int(sizes[best]), int(count)


# ------------------------------------------------------------------------------------------------ K30b
def convex_hull(points):
    """Distinct integer points (x, y) → the strictly convex hull (collinear points dropped), counter-clockwise: one point for
    one, two for collinear ones."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) <= 1:
        return pts

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def canonical(ex, ey):
    """e turned by multiples of 90 degrees to ex > 0, -ex < ey <= ex."""
    for _ in range(4):
        if ex > 0 and -ex < ey <= ex:
            return ex, ey
        ex, ey = -ey, ex
    raise ValueError('the zero vector has no direction')


def _extents(hull, ex, ey):
    u = [x * ex + y * ey for x, y in hull]
    v = [ex * y - ey * x for x, y in hull]
    return min(u), max(u), min(v), max(v)


def chosen_direction(hull):
    """The canonical direction of the hull edge whose rectangle is the smallest: the key is (area as a Fraction, |ey| / ex
    as a Fraction, ey < 0), all exact."""
    best = None
    for i, a in enumerate(hull):
        b = hull[(i + 1) % len(hull)]
        ex, ey = b[0] - a[0], b[1] - a[1]
        umin, umax, vmin, vmax = _extents(hull, ex, ey)
        cx, cy = canonical(ex, ey)
        key = (Fraction((umax - umin) * (vmax - vmin), ex * ex + ey * ey), Fraction(abs(cy), cx), cy < 0)
        if best is None or key < best[0]:
            best = (key, (cx, cy))
    return best[1], best[0][0]


def candidates(mask):
    """Per image row the leftmost and the rightmost set cell, as (x, y): they suffice as candidates for the hull."""
    mask = np.asarray(mask, dtype=bool)
    ys = np.flatnonzero(mask.any(axis=1))
    left = mask[ys].argmax(axis=1)
    right = mask.shape[1] - 1 - mask[ys, ::-1].argmax(axis=1)
    return list(zip(left.tolist(), ys.tolist())) + list(zip(right.tolist(), ys.tolist()))


def min_area_box(mask):
    """mask (H, W) bool → (n, hull vertex count, box (5,) f64 = cx, cy, dx, dy, theta) in cell units, over ALL set cells."""
    ys, xs = np.nonzero(np.asarray(mask, dtype=bool))
    n = int(xs.size)
    if n == 0:
        return 0, 0, np.zeros(5)
    hull = convex_hull(candidates(mask))
    if len(hull) == 1:
        return n, 1, np.array([hull[0][0], hull[0][1], 1.0, 1.0, 0.0])
    (ex, ey), _ = chosen_direction(hull)
    umin, umax, vmin, vmax = _extents(hull, ex, ey)
    theta = np.arctan2(np.float64(ey), np.float64(ex))
    c, s, length = np.cos(theta), np.sin(theta), np.sqrt(np.float64(ex * ex + ey * ey))
    cell = abs(c) + abs(s)
    uc, vc = 0.5 * np.float64(umax + umin) / length, 0.5 * np.float64(vmax + vmin) / length
    return n, len(hull), np.array([uc * c - vc * s, uc * s + vc * c, np.float64(umax - umin) / length + cell,
                                   np.float64(vmax - vmin) / length + cell, theta])


def through_centres_area(mask):
    """The exact area (a Fraction) of the chosen rectangle through the cells' centres, without the unit-cell support."""
    hull = convex_hull(candidates(mask))
    return chosen_direction(hull)[1] if len(hull) >= 2 else Fraction(0)


# ------------------------------------------------------------------------------------------------ the cases both test files use
def rect(h, w, cx, cy, length, width, deg):
    """Cells whose centre lies in the rectangle (numpy paint), as the K25 test paints them."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.deg2rad(deg)
    u = (xs - cx) * np.cos(a) + (ys - cy) * np.sin(a)
    v = (ys - cy) * np.cos(a) - (xs - cx) * np.sin(a)
    return (np.abs(u) <= length / 2) & (np.abs(v) <= width / 2)


def rotated_rectangles():
    """The twelve rotated rectangles of the K25 test (64 x 64, 7 + 15 k degrees, aspect >= 2.5), by name."""
    h = w = 64
    return {f'rect{deg:g}': rect(h, w, w / 2 + 0.3 * k, h / 2 - 0.2 * k, 30 + k, 8 + (k % 5), deg)
            for k, deg in enumerate(np.arange(12) * 15 + 7.0)}


def ell(h=40, w=36):
    m = np.zeros((h, w), dtype=bool)
    m[5:30, 5:10] = True
    m[25:30, 5:30] = True
    return m


def block(h=40, w=36):
    m = np.zeros((h, w), dtype=bool)
    m[5:12, 4:25] = True
    return m


def line(h=40, w=36):
    m = np.zeros((h, w), dtype=bool)
    m[3:h - 2, 7] = True
    return m


def single(h=40, w=36):
    m = np.zeros((h, w), dtype=bool)
    m[h - 1, w - 1] = True
    return m


def diamond(h=64, w=64, cx=30, cy=33, r=9):
    """|x - cx| / 2 + |y - cy| <= r: symmetric about both axes, so the edges (2, 1) and (2, -1) tie in area and in |ey| / ex."""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.abs(xs - cx) + 2 * np.abs(ys - cy) <= 2 * r


# the grids of the GPU test.  (33, 33) is the spiral's.  (160, 160) is there for the Bernoulli masks: at p = 0.6 a mask needs
# that many cells to fall into 20 components.  (130, 1000) is the smallest grid whose row-aligned plane (130 rows of 32 words)
# exceeds the 4096 words K30a keeps in LDS: masks with a large bounding box take the workspace path there, small ones do not.
GRIDS = ((40, 36), (64, 64), (33, 100), (33, 33), (1, 40), (40, 1), (1, 1), (160, 160), (130, 1000))


def spiral(n=33):
    """A one-cell-wide square spiral with a one-cell gap between its turns: one component with a long geodesic path."""
    m = np.zeros((n, n), dtype=bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    for _ in range(n * n):
        ny, nx = y + dy, x + dx
        ahead = (ny + dy, nx + dx)
        blocked = not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or \
            (0 <= ahead[0] < n and 0 <= ahead[1] < n and m[ahead])
        if blocked:
            dy, dx = dx, -dy                                           # turn right
            ny, nx = y + dy, x + dx
            ahead = (ny + dy, nx + dx)
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ahead[0] < n and 0 <= ahead[1] < n and m[ahead]):
                break
        y, x = ny, nx
        m[y, x] = True
    return m


def component_masks(h, w):
    """The K30a cases that fit an (h, w) grid, by name."""
    m = {'empty': np.zeros((h, w), dtype=bool), 'full': np.ones((h, w), dtype=bool)}
    m['single'] = np.zeros((h, w), dtype=bool)
    m['single'][h - 1, w - 1] = True                                   # the last pixel of the map
    m['checkerboard'] = (np.add.outer(np.arange(h), np.arange(w)) % 2).astype(bool)     # one component when h, w >= 2
    if h >= 33 and w >= 33:
        z = np.zeros((h, w), dtype=bool)
        m['corner'] = z.copy()
        m['corner'][4:9, 3:8] = m['corner'][9:12, 8:20] = True         # two blobs touching only at a corner: one component
        m['equal'] = z.copy()
        m['equal'][20:24, 2:7] = m['equal'][3:8, w - 6:w - 2] = True   # 20 cells each: the upper right one comes first
        m['strays'] = rect(h, w, w / 2, h / 2, 30, 9, 7.0)             # the rectangle of the issue's example ...
        m['strays'][2, w - 4] = m['strays'][h - 3, 3] = True           # ... plus two stray cells
        m['ring'] = z.copy()
        m['ring'][5:25, 5:25] = True
        m['ring'][8:22, 8:22] = False
        m['ring'][12:18, 12:18] = True                                 # a separate blob inside the hole
        for k, p in enumerate((0.3, 0.45, 0.6)):
            m[f'bernoulli{p:g}'] = np.random.default_rng(300 + k).random((h, w)) < p
    if h * w > 100000:                                                 # the workspace grid: what takes each path there is enough
        m = {k: m[k] for k in ('empty', 'full', 'single', 'corner', 'equal', 'strays', 'bernoulli0.45')}
    if (h, w) == (33, 33):
        m['spiral'] = spiral(33)
    if (h, w) == (33, 100):
        m['wide'] = rect(h, w, 50.2, 16.4, 90, 9, 12)                  # crosses several word boundaries in every row
        m['wide'][0, 31:34] = m['wide'][32, 95:100] = True
    return m


def rectangle_masks(h, w):
    """The K30b cases that fit an (h, w) grid, by name."""
    m = {'empty': np.zeros((h, w), dtype=bool)}
    if (h, w) == (64, 64):
        m.update(rotated_rectangles())
        m['diamond'] = diamond()
        m['diagonal'] = np.zeros((h, w), dtype=bool)
        m['diagonal'][np.arange(10, 30), np.arange(40, 20, -1)] = True  # collinear cells off the axes
    if (h, w) == (40, 36):
        m.update(ell=ell(), line=line(), single=single(), block=block())
    return m
