"""CPU side of tests/test_k17_paths_gpu.py: operands as a 16-bit type holds them, the float64 / float32 evaluations of K17's
products and epilogues (the float32 one sets the bar, f64_bars.f32_bar), and plain-Python restatements of the host rules of
csrc/gemm.hip that decide which kernel a shape runs (block shape, split of a contraction, partial-row layout, grouped depth).
Plain torch on the CPU; nothing here touches the device or the library."""
import math

import torch

F32, F64 = torch.float32, torch.float64
KB, NS = 32, 3                    # K-step depth and ring slots of csrc/gemm.hip
TN_GROUP, TN_GROUP_DEPTH = 48, 4096
SENTINEL = 0x7FC12345             # a NaN payload: no kernel writes it, and no float compares equal to it


def ceil_div(a, b):
    return -(-a // b)


# ---- operands -------------------------------------------------------------------------------------------------------
def randn(seed, shape, dt, scale=1.0):
    """N(0, scale^2) drawn on the CPU with a seeded generator and rounded to ``dt``; returned in ``dt``."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


def exact16(t):
    """``t`` rounded to values bf16 AND fp16 hold exactly (8 significant bits, normal in fp16): one reference serves both."""
    t = t.to(torch.bfloat16).float()
    t[t.abs() < 2.0 ** -14] = 0.0
    return t


def column_block(t, ld, at):
    """``t`` (rows, n) as columns at : at + n of a (rows, ld) matrix of zeros-free filler: a row stride that is not ``n``."""
    big = torch.full((t.shape[0], ld), 3.0, dtype=t.dtype)
    big[:, at:at + t.shape[1]] = t
    return big


# ---- float64 / float32 evaluations -----------------------------------------------------------------------------------
def gelu(z):
    return torch.nn.functional.gelu(z)          # the exact erf form, in the dtype of z


def dgelu(z):
    """d gelu / dz = Phi(z) + z phi(z), exact erf form."""
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def act(kind, z):
    return {None: lambda v: v, 'relu': torch.relu, 'gelu': gelu}[kind](z)


def dact(kind, z):
    return (z > 0).to(z.dtype) if kind == 'relu' else dgelu(z)


def both(fn, *ts):
    """``fn`` on the float64 and on the float32 copies of ``ts`` (None passes through): (ref64, ref32)."""
    return tuple(fn(*[None if t is None else t.to(fdt) for t in ts]) for fdt in (F64, F32))


# ---- host rules of csrc/gemm.hip, restated -----------------------------------------------------------------------------
def tile_rows(atomic, gm, gn, work_units):
    """gemm16_pick_shape: the rows of the block tile (128 | 256; columns are 128 either way) of a (gm x gn) output with
    ``work_units`` batch items.  256 x 128 when the product stores, wastes at most 10 % more of its tiles on the edges than
    128 x 128 does, and has at least 128 such tiles."""
    def eff(bm):
        return (gm * gn) / (ceil_div(gm, bm) * bm * ceil_div(gn, 128) * 128)

    def blocks(bm):
        return ceil_div(gm, bm) * ceil_div(gn, 128) * work_units
    if atomic:
        return 128
    return 256 if eff(256) >= 0.9 * eff(128) and blocks(256) >= 128 else 128


def nn_part_rows(m, k, batch=1):
    """mbv_gemm16_nn_part_rows: one partial column-sum row per 64 output rows (a wave row) of every row tile."""
    bm = tile_rows(0, m, k, batch)
    return (bm // 64) * ceil_div(m, bm) * batch


def nn_dead_part_rows(m, k):
    """Partial rows whose 64 output rows lie wholly beyond m (wave rows of the last row tile with nothing to sum)."""
    return [r for r in range(nn_part_rows(m, k)) if 64 * r >= m]


def nn_workspace_bytes(m, k, batch=1):
    return (ceil_div(m, 64) + 4) * k * 4 * max(batch, 1)


def ring_steps(contraction):
    """(K-steps of one part, whether the last is ragged)."""
    return ceil_div(contraction, KB), contraction % KB != 0


def split(contraction, tiles, splits=0):
    """gemm16_split: (parts, K-steps per part) of an accumulating product — about 512 workgroups, parts at least 256 deep."""
    total = ceil_div(contraction, KB)
    s = splits
    if s <= 0:
        s = min(ceil_div(512, tiles), total * KB // 256)
    s = min(max(s, 1), total)
    ksteps = ceil_div(total, s)
    return ceil_div(total, ksteps), ksteps


def tn_acc_route(m, n, k, contiguous):
    """mbv_gemm16_tn with accumulate = 1, batch 1, the wrapper's workspace: ('owner' | 'atomic-finish' | 'atomics', parts).
    owner: stored parts, k_add_parts with gridDim.y == 1; atomic-finish: stored parts, k_add_parts cut into part ranges that end
    in f32 atomics; atomics: the GEMM's own f32 atomic adds."""
    parts, _ = split(m, ceil_div(n, 128) * ceil_div(k, 128))
    if parts > 1 and contiguous:
        return ('atomic-finish' if n * k < 65536 and parts >= 32 else 'owner'), parts
    return 'atomics', parts


def tn_workspace_bytes(m, n, k):
    tiles = ceil_div(n, 128) * ceil_div(k, 128)
    s = max(min(ceil_div(512, tiles), ceil_div(m, 256)), 1)
    return (s + 1) * n * k * 4


def tn_group_parts(m):
    """tn_group_split: token ranges of one grouped entry (1: the owner adds its tile to dw in place, ``acc_out``)."""
    total = ceil_div(m, KB)
    s = max(ceil_div(m, TN_GROUP_DEPTH), 1)
    return ceil_div(total, ceil_div(total, s))
