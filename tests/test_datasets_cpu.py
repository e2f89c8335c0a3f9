"""CPU tests of what the on-disk readers of mask_bev_amd/datasets.py share: which samples a rank gets and in which order an
epoch visits them."""
import torch


def test_shard_drops_the_remainder_and_strides_by_rank():
    from mask_bev_amd.datasets import shard
    items = list(range(11))                        # 11 - 11 % (2 * 2) = 8 usable
    assert shard(items, 0, 2, 2) == [0, 2, 4, 6]
    assert shard(items, 1, 2, 2) == [1, 3, 5, 7]
    assert shard(items, 0, 1, 1) == items and shard(items[:3], 0, 2, 2) == []


def test_epoch_order():
    from mask_bev_amd.datasets import epoch_order
    assert list(epoch_order(7, 3, False)) == list(range(7))
    for epoch in (0, 5):
        want = torch.randperm(7, generator=torch.Generator().manual_seed(epoch)).tolist()
        assert list(epoch_order(7, epoch, True)) == want
    assert list(epoch_order(7, 0, True)) != list(epoch_order(7, 5, True))
