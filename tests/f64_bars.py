"""Shared pieces of the per-kernel float64 suites (test_k4_paths_gpu.py, test_k6_paths_gpu.py, test_k7_paths_gpu.py, and the
encoder front: test_k2_paths_gpu.py — PillarFeatureNet, with its dense reference tests/pfn_ref.py — and test_k3_paths_gpu.py —
scatter + LayerNorm; and the normalisation kernels: test_k12_paths_gpu.py, test_k18_paths_gpu.py, with tests/norm_ref.py; and the decoder's row chains: test_k19_paths_gpu.py, with tests/decoder_ref.py): the relative max-norm error, the printed ``err … bar …`` line, roundings of a float64 tensor to a 16-bit
type and the project's f32 bar."""
import torch

F32_BAR = 4e-6                                            # the project's f32 bar (test_k5_msda_paths_gpu.py)
LO = (torch.bfloat16, torch.float16)
ROUNDING = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # one rounding: half an ulp, relative
NAME = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'fp16'}


def err(got, ref) -> float:
    """max|got - ref| / max|ref| in float64 on the CPU."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max())


def report(capsys, module, tag, e, bar):
    with capsys.disabled():
        print(f'\n[{module}] {tag}: err {e:.3e} bar {bar:.3e}', end='')


def check(capsys, module, tag, e, bar, bad):
    """Print the comparison; a miss is collected in ``bad`` (asserted empty by the caller, after every line is printed)."""
    report(capsys, module, tag, e, bar)
    if not e <= bar:
        bad.append(f'{tag}: {e:.3e} > {bar:.3e}')


def f32_bar(ref32, ref64) -> float:
    """max(4e-6, 4 x the float32 CPU reference's own error): 4x covers summation order and FMA differences."""
    return max(F32_BAR, 4.0 * err(ref32, ref64))


def rd(t, dt):
    """``t`` (float64) rounded to ``dt`` and back: one rounding point of a kernel."""
    return t.to(dt).to(t.dtype)


def half_ulp(x, dt):
    """Half an ulp of |x| (float64) in ``dt`` — one rounding (a value within 2^-20 of a binade's end may sit in the next)."""
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dt]
    a = (x.abs() * (1 + 2.0 ** -20)).clamp_min(2.0 ** emin)
    return torch.exp2(torch.floor(torch.log2(a)) - mant) / 2


def err_beyond_one_rounding(got, ref64, dt) -> float:
    """max(|got - ref64| - one rounding of ref64 to ``dt``) / max|ref64|: what a 16-bit stored result of an f32-accumulated
    product may add to the f32 bar."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    return float(((got - ref64).abs() - half_ulp(ref64, dt)).max() / ref64.abs().max())


class RoundGrad(torch.autograd.Function):
    """Identity whose gradient is rounded to ``dt``: a gradient the kernel stores in the 16-bit type."""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return rd(g, ctx.dt), None


class RoundValue(torch.autograd.Function):
    """Rounding to ``dt`` whose gradient passes through: a high-precision parameter the kernel stages in the 16-bit type."""

    @staticmethod
    def forward(ctx, x, dt):
        return rd(x, dt)

    @staticmethod
    def backward(ctx, g):
        return g, None
