"""tests/norm_ref.py (the case builders and CPU references of test_k12_paths_gpu.py and test_k18_paths_gpu.py) on its own, without a
GPU: the ReLU cases leave no element within f32 rounding of a flipped gate, the float32 reference's own error keeps every bar
under the cap at the offset inputs, and the builders state the operations they claim to."""
import pytest
import torch
import torch.nn.functional as F

from tests import norm_ref as R
from tests.f64_bars import NAME, f32_bar
from tests.norm_ref import F32, F64


@pytest.mark.parametrize('x_dt', sorted({d[0] for d in R.GN_DTYPES}, key=str), ids=lambda d: NAME[d])
@pytest.mark.parametrize('ci', range(len(R.GN_CASES)), ids=R.GN_IDS)
def test_relu_cases_have_no_gate_within_rounding_of_zero(ci, x_dt):
    k = R.gn_inputs(ci, 'n0.3', x_dt, x_dt)
    assert R.relu_band(k.x, k.w, k.bias, k.groups) == 0
    y = F.group_norm(k.x.double(), k.groups, k.w.double(), k.bias.double(), R.EPS)
    assert 0.2 < float((y > 0).double().mean()) < 0.8                    # both sides of the gate are populated


def test_relu_band_counts_what_it_says():
    x = torch.tensor([[-1.0, 1.0, -1.0, 1.0]]).view(1, 1, 2, 2)          # mean 0, rstd 1 - 5e-6: y = x rstd + beta
    one, rstd = torch.ones(1), float(R.gn_stats(x, 1)[1])
    assert R.relu_band(x, one, torch.tensor([rstd]), 1) == 2             # the two -1 land on zero
    assert R.relu_band(x, one, torch.tensor([0.5]), 1) == 0


def test_conv_gn_case_has_no_gate_within_rounding_of_zero():
    k = R.conv_gn_inputs()
    ref = R.conv_gn_reference(k)
    up = F.interpolate(k.add.double(), size=(24, 16), mode='bilinear', align_corners=False)
    assert R.relu_band(ref[F64]['z'], k.w, k.bias, k.groups, add=up) == 0
    assert all(f32_bar(ref[F32][n], ref[F64][n]) <= R.BAR_CAP for n in ('y', 'dx', 'dcw', 'dw', 'dbias', 'dadd'))


@pytest.mark.parametrize('ci', range(len(R.GN_CASES)), ids=R.GN_IDS)
def test_offset_bars_stay_under_the_cap(ci):
    """torch's float32 GroupNorm on N(50, 1): its error against float64, times 4, is a bar under 1e-5 for y, dx and d beta; its
    d gamma cancels at that offset, and norm_ref.bar holds that bar at the cap."""
    k = R.gn_inputs(ci, 'n50', F32, F32)
    ref = R.gn_reference(k.x, k.w, k.bias, k.groups, k.gy)
    for n in ('y', 'dx', 'dbias'):
        assert f32_bar(ref[F32][n], ref[F64][n]) <= R.BAR_CAP, n
    assert f32_bar(ref[F32]['dw'], ref[F64]['dw']) > R.BAR_CAP and R.bar(ref[F32]['dw'], ref[F64]['dw']) == R.BAR_CAP
    mean, rstd = R.gn_stats(k.x, k.groups)
    assert float((mean - 50).abs().max()) < 0.5 and float((rstd - 1).abs().max()) < 0.5


def test_add_sizes():
    assert [R.gn_add_size(kd, 92, 92) for kd in R.GN_ADDS] == [(46, 46), (31, 23), (1, 1), (92, 92)]
    assert R.gn_inputs(1, 'n0.3', F32, F32).adds == {}                   # W = 6: no fused add


def test_unfold_order_and_position_map():
    x = torch.arange(2 * 4 * 6 * 3, dtype=F64).view(2, 4, 6, 3)
    u = R.unfold2x2(x)
    assert tuple(u.shape) == (2, 2, 3, 12)
    for c in range(3):
        for kh in range(2):
            for kw in range(2):
                assert torch.equal(u[..., c * 4 + kh * 2 + kw], x[:, kh::2, kw::2, c])
    ape = torch.arange(5 * 7 * 2, dtype=F64).view(1, 2, 7, 5)           # (rows, cols) = (w, h) as the model has it
    t = R.pos_map(5, 7, 2)(ape)
    assert tuple(t.shape) == (1, 5, 7, 2) and torch.equal(t.reshape(35, 2), ape.view(2, 35).t())


@pytest.mark.parametrize('c', [192, 768])
def test_value_rows_with_exact_sums_give_beta(c):
    a = R.ln_value_rows(7, c)
    k = R.ln_inputs(8, (64, c), b_dt=None)
    ref = R.ln_reference(a, None, k.w, k.bias, (k.g1,))
    for dt in (F64, F32):
        for row in (R.VALUE_ROWS['zeros'], R.VALUE_ROWS['half']):
            assert torch.equal(ref[dt]['y'][row], k.bias.to(dt))
    assert float((a[R.VALUE_ROWS['offset']].mean() - 50).abs()) < 0.1
    assert all(f32_bar(ref[F32][n], ref[F64][n]) <= R.BAR_CAP for n in ('y', 'da', 'dw', 'dbias'))


def test_ln_reference_sums_the_upstream_gradients_and_the_branch():
    k = R.ln_inputs(3, (5, 8))
    two = R.ln_reference(k.a, k.b, k.w, k.bias, (k.g1, k.g2), k.g3)[F64]
    one = R.ln_reference(k.a, k.b, k.w, k.bias, (k.g1.double() + k.g2.double(),), k.g3)[F64]
    assert torch.equal(two['da'], one['da']) and torch.equal(two['da'], two['db'])
    assert torch.allclose(two['dbranch'], two['da'].sum(0), rtol=0, atol=0)
    only_s = R.ln_reference(k.a, k.b, k.w, k.bias, (), k.g3)[F64]
    assert torch.equal(only_s['da'], k.g3.double()) and only_s['dw'] is None
