"""Inference API on the host: Predictions helpers on hand-made packed words, the K21 ABI names, CPU tensors refused."""
import pytest
import torch

from tests.util_cfg import random_scans, tiny_kwargs


def _pack(dense):
    """(N, H, W) bool → words in the mbv_pack_binary_masks layout (pixel p at bit p % 32 of word p // 32, 64-pixel groups)."""
    n, h, w = dense.shape
    flat = dense.reshape(n, -1)
    words = ((h * w + 63) // 64) * 2
    pad = torch.zeros(n, words * 32, dtype=torch.bool)
    pad[:, :h * w] = flat
    bits = pad.view(n, words, 32).long() << torch.arange(32)
    w64 = bits.sum(-1)
    return torch.where(w64 >= 2 ** 31, w64 - 2 ** 32, w64).to(torch.int32)


@pytest.mark.parametrize('h,w', [(5, 7), (4, 32), (3, 41), (8, 64)])
def test_unpack_bits_round_trip(h, w):
    from mask_bev_amd.predict import unpack_bits
    g = torch.Generator().manual_seed(h * w)
    dense = torch.rand(3, h, w, generator=g) > 0.5
    dense[0, -1, -1] = True                       # the last pixel (bit 31 of a word when h*w % 32 == 0: a negative int32)
    assert torch.equal(unpack_bits(_pack(dense), h, w), dense)


def test_hand_made_words():
    from mask_bev_amd.predict import unpack_bits
    # 2 x 41 grid: pixel (1, 0) is linear index 41 = bit 9 of word 1; pixel (0, 31) = bit 31 of word 0
    words = torch.zeros(1, 4, dtype=torch.int32)
    words[0, 1] = 1 << 9
    words[0, 0] = -2 ** 31
    m = unpack_bits(words, 2, 41)
    assert m.sum() == 2 and m[0, 1, 0] and m[0, 0, 31]


def test_instances_lists_kept_queries():
    from mask_bev_amd import ops
    from mask_bev_amd.predict import Predictions
    B, Q, H, W = 2, 3, 3, 41
    dense = torch.zeros(B * Q, H, W, dtype=torch.bool)
    dense[1, 2, 40] = True
    dense[1, 0, :3] = True
    dense[5, 1, 1] = True
    labels = torch.tensor([[0, 2, 1], [1, 0, 3]], dtype=torch.int32)
    scores = torch.tensor([[0.9, 0.8, 0.3], [0.6, 0.99, 0.7]])
    keep = torch.tensor([[False, True, False], [True, False, True]])
    areas = dense.flatten(1).sum(1).view(B, Q).to(torch.int32)
    ms = torch.rand(B, Q)
    p = Predictions(labels, scores, keep, ops.PackedMasks(_pack(dense), H, W), areas, ms,
                    torch.full((B, H, W), -1, dtype=torch.int32), (H, W))
    i0 = p.instances(0)
    assert [d['query'] for d in i0] == [1] and i0[0]['label'] == 2 and i0[0]['area'] == 4
    assert torch.equal(i0[0]['mask'], dense[1]) and abs(i0[0]['score'] - 0.8) < 1e-7
    i1 = p.instances(1)
    assert [d['query'] for d in i1] == [0, 2] and torch.equal(i1[1]['mask'], dense[5]) and i1[1]['area'] == 1
    c = p.clone()
    assert c.masks.words is not p.masks.words and torch.equal(c.masks.words, p.masks.words)
    assert p.cpu().labels.device.type == 'cpu'
    nomask = Predictions(labels, scores, keep, None, None, None, None, (H, W))
    assert nomask.instances(1)[0]['mask'] is None


def test_k21_names_in_signatures():
    from mask_bev_amd import _lib
    for name in ('mbv_select_queries', 'mbv_extract_masks_workspace_bytes', 'mbv_extract_masks'):
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 59


def test_cpu_tensors_are_refused():
    from mask_bev_amd._lib import MaskBevHipError
    from mask_bev_amd.mask_bev_module import MaskBevModule
    from mask_bev_amd.predict import extract_instances
    with pytest.raises(MaskBevHipError):
        extract_instances(torch.zeros(1, 4, 3), torch.zeros(1, 4, 8, 8), (32, 32))
    kw = tiny_kwargs(nx=32, ny=32, q=4)
    m = MaskBevModule(**kw)
    was = m.training
    with pytest.raises(MaskBevHipError):
        m.predict(random_scans(kw, [100], seed=0))
    assert m.training == was
