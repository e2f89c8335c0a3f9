"""ops_pgrad without a device or the library: which gradient `arena_grad` hands out, how `_distinct_destination_waves`
keeps a destination from meeting itself in one grouped launch, and what the deferred-work records carry."""
import torch

from mask_bev_amd import ops_pgrad as P


def _param(grad_dtype=torch.float32, arena=True):
    p = torch.nn.Parameter(torch.zeros(7, 4, dtype=grad_dtype or torch.float32))     # (a gradient has its tensor's dtype)
    if grad_dtype is not None:
        p.grad = torch.zeros(7, 4, dtype=grad_dtype)
    if arena:
        p._mbv_arena = True
    return p


def test_arena_grad_is_the_f32_gradient_of_an_arena_parameter_only():
    assert P.arena_grad(None) is None
    p = _param()
    assert P.arena_grad(p) is p.grad
    assert P.arena_grad(_param(arena=False)) is None                  # a plain tensor without the flag
    assert P.arena_grad(_param(grad_dtype=None)) is None              # no gradient
    assert P.arena_grad(_param(grad_dtype=torch.bfloat16)) is None    # a gradient that is not f32
    assert P.arena_grad(_param(grad_dtype=torch.bfloat16), rows=(2, 5)) is None


def test_arena_grad_rows_is_a_view_of_the_gradient():
    p = _param()
    g = P.arena_grad(p, rows=(2, 5))
    assert tuple(g.shape) == (3, 4)
    assert g.untyped_storage().data_ptr() == p.grad.untyped_storage().data_ptr()
    assert g.data_ptr() == p.grad[2].data_ptr()
    g += 1.0                                                          # writes through: never a copy
    assert float(p.grad[2:5].sum()) == 12.0 and float(p.grad.sum()) == 12.0


def test_distinct_destination_waves():
    buf = torch.zeros(12, 4)
    g, x = torch.zeros(3, 6), torch.zeros(3, 4)
    a, b, c = buf[0:6], buf[6:12], torch.zeros(6, 4)
    first, again, other, third, lone = (g, x, a), (g, x, a), (g, x, b), (g, x, a), (g, x, c)
    waves = P._distinct_destination_waves([first, again, other, third, lone])
    # two products into the same acc land in successive waves; disjoint row slices of one buffer share a wave; order within
    # a wave is the input order
    assert len(waves) == 3
    assert [id(it) for it in waves[0]] == [id(first), id(other), id(lone)]
    assert [id(it) for it in waves[1]] == [id(again)]
    assert [id(it) for it in waves[2]] == [id(third)]
    overlap = (g, x, buf[3:9])                                        # overlaps both halves: a wave of its own
    waves = P._distinct_destination_waves([first, other, overlap])
    assert [[id(it) for it in w] for w in waves] == [[id(first), id(other)], [id(overlap)]]
    assert P._distinct_destination_waves([]) == []


def test_records_built_from_a_small_f32_record():
    g = torch.zeros(5, 24)[:, 8:16]                                   # a column block: row stride 24
    x, acc, bias_acc, stream = torch.zeros(5, 4), torch.zeros(8, 4), torch.zeros(8), object()
    small = P.SmallWgrad(g, x, acc, bias_acc, stream)
    assert small._fields == ('g', 'x', 'acc', 'bias_acc', 'stream')
    cs = P._small_bias_colsum(small)
    assert isinstance(cs, P.ColSum) and cs._fields == ('g', 'out', 'rows', 'n', 'ld', 'offset', 'stream')
    assert cs.g is g and cs.out is bias_acc and cs.stream is stream
    assert (cs.rows, cs.n, cs.ld, cs.offset) == (g.shape[0], g.shape[1], g.stride(0), 0) == (5, 8, 24, 0)
    k20 = P._small_as_k20(small)
    assert isinstance(k20, P.K20Wgrad) and k20._fields == ('g', 'x', 'acc', 'amax_g', 'amax_x', 'stream')
    assert k20.g is g and k20.x is x and k20.acc is acc and k20.stream is stream
    assert k20.amax_g is None and k20.amax_x is None
    assert P.K17Wgrad._fields == ('g', 'x', 'acc', 'stream')
    lists = P.PendingPass([], [], [], [])
    assert lists._fields == ('small', 'colsum', 'tn', 'tn32') and not any(lists)
    lists.colsum.append(cs)
    assert any(lists)
