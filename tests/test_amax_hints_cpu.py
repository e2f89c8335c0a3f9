"""The bookkeeping of K20's absmax HINTS (mask_bev_amd/ops_records.py) on CPU tensors: a record belongs to ONE tensor object
while that object is unmodified, in the capture state it was made in.  Views find their owner's record through ``_base``;
another tensor — whatever its address — finds none."""
import torch

from mask_bev_amd import ops_records as R

TAG = 0


def _hinted(shape=(8, 6)):
    t, rec = torch.randn(shape), torch.zeros((1, R.AMAX_SLOTS), dtype=torch.int32)
    R._hint_set(t, rec, TAG)
    return t, rec


class _Fresh(torch.autograd.Function):
    """Leaves a hint on a fresh output (and on a second one it saves: re-read in backward, that one is a new object)."""
    seen = None

    @staticmethod
    def forward(ctx, x, rec):
        y, a = x * 2, x + 1
        R._hint_set(y, rec, TAG)
        R._hint_set(a, rec, TAG)
        ctx.save_for_backward(a)
        return y, a

    @staticmethod
    def backward(ctx, gy, ga):
        _Fresh.seen = R._hint_get(ctx.saved_tensors[0], TAG)
        return gy * 2 + ga, None


class _Dirty(torch.autograd.Function):
    """Writes a caller-owned buffer and returns it through mark_dirty (K3's ``out``)."""

    @staticmethod
    def forward(ctx, x, out, rec):
        ctx.mark_dirty(out)
        out.data.copy_(x)
        R._hint_set(out, rec, TAG)
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None, None


def test_the_object_and_its_views_find_the_record():
    t, rec = _hinted()
    assert R._hint_get(t, TAG) is rec
    assert R._hint_get(t.view(2, 4, 6), TAG) is rec                  # a view of the whole tensor
    assert R._hint_get(t[2:5], TAG) is rec                           # a row slice: the whole tensor's record bounds it
    assert R._hint_get(t.view(2, 4, 6)[1].reshape(-1, 3), TAG) is rec          # a view of a view
    # set through a whole-tensor view, the record lives with the tensor
    u, rec2 = torch.randn(8, 6), torch.ones((1, R.AMAX_SLOTS), dtype=torch.int32)
    R._hint_set(u.view(-1, 3), rec2, TAG)
    assert R._hint_get(u, TAG) is rec2 and R._hint_get(u.view(48), TAG) is rec2


def test_function_outputs_keep_the_record_their_forward_set():
    rec = torch.zeros((1, R.AMAX_SLOTS), dtype=torch.int32)
    x = torch.randn(8, 6, requires_grad=True)
    y, a = _Fresh.apply(x, rec)
    assert R._hint_get(y, TAG) is rec and R._hint_get(a, TAG) is rec
    out = torch.empty(8, 6)
    got = _Dirty.apply(x, out, rec)
    assert R._hint_get(got, TAG) is None                             # mark_dirty bumped the version behind the forward's hint
    R.amax_hint_restamp(got)
    assert R._hint_get(got, TAG) is rec and R._hint_get(got.view(-1, 3), TAG) is rec


def test_other_tensors_and_modified_tensors_find_none():
    t, rec = _hinted()
    assert R._hint_get(t.clone(), TAG) is None
    assert R._hint_get(t.detach(), TAG) is None                      # a new object without a _base: carried by hand where needed
    assert R._hint_get(t, TAG + 1) is None                           # another capture state / generation
    assert R._hint_get(t, TAG) is rec
    t.add_(1.0)
    assert R._hint_get(t, TAG) is None and R._hint_get(t[:2], TAG) is None
    t, rec = _hinted()
    t.view(-1, 3)[5].zero_()                                         # an in-place write through a view
    assert R._hint_get(t, TAG) is None
    # a saved OUTPUT re-read in backward is a new object: the Function carries its record in ctx instead
    x = torch.randn(8, 6, requires_grad=True)
    y, a = _Fresh.apply(x, rec)
    _Fresh.seen = 'unset'
    (y.sum() + a.sum()).backward()
    assert _Fresh.seen is None


def test_restamp_cannot_give_a_record_to_an_object_that_has_none():
    t, rec = _hinted()
    other = torch.empty_like(t)
    R.amax_hint_restamp(other)
    assert R._hint_get(other, TAG) is None
    got = _Dirty.apply(torch.randn(8, 6, requires_grad=True), other, None)     # a forward that sets no hint
    R.amax_hint_restamp(got)
    assert R._hint_get(got, TAG) is None
    # ... also when the buffer carried an older record: the forward that overwrote it dropped that one
    assert R._hint_get(t, TAG) is rec
    got = _Dirty.apply(torch.randn(8, 6, requires_grad=True), t, None)
    R.amax_hint_restamp(got)
    assert R._hint_get(got, TAG) is None and R._hint_get(t, TAG) is None


def test_public_functions_gate_on_the_device():
    t = torch.randn(8, 6)
    R.amax_hint_set(t, torch.zeros((1, R.AMAX_SLOTS), dtype=torch.int32))     # a CPU tensor takes no hint
    assert R.amax_hint_get(t) is None
