"""The table-sum form of the two code-fed layers (tests/code_tables_spec.py) against the layers themselves in float64:
pins the tap, phase and padding algebra of the tables, which is what a transposed-convolution table most easily gets
wrong.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import code_tables_spec as S

MAPS = [(1, 1), (1, 3), (3, 5), (4, 4)]
K, D, C3, CU = 12, 8, 12, 8


def _case(seed):
    g = torch.Generator().manual_seed(seed)
    w3 = torch.randn(C3, D, 3, 3, generator=g, dtype=torch.float64)
    wT = torch.randn(D, CU, 4, 4, generator=g, dtype=torch.float64)
    e = torch.randn(K, D, generator=g, dtype=torch.float64)
    b3 = torch.randn(C3, generator=g, dtype=torch.float64)
    bU = torch.randn(CU, generator=g, dtype=torch.float64)
    return g, w3, wT, e, b3, bU


@pytest.mark.parametrize("hw", MAPS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("B", [1, 3])
def test_table_sums_equal_the_layers(hw, B):
    g, w3, wT, e, b3, bU = _case(3)
    H, W = hw
    ids = torch.randint(0, K, (B, H, W), generator=g)
    ids.view(-1)[0], ids.view(-1)[-1] = 0, K - 1
    q = e[ids].permute(0, 3, 1, 2)                       # the quantised map [B, D, H, W]
    t3, tu = S.tables(w3, wT, e)
    got3, mag3, bad3 = S.conv3_sum(t3, b3, ids, relu=False)
    ref3 = F.conv2d(q, w3, b3, padding=1).permute(0, 2, 3, 1)
    assert (got3 - ref3).abs().max() <= 1e-12 * ref3.abs().max()
    assert not bad3.any() and (mag3 >= got3.abs() - 1e-9).all()
    gotr, _, _ = S.conv3_sum(t3, b3, ids, relu=True)
    assert torch.equal(gotr, torch.relu(got3))
    gotU, magU, badU = S.upsample_sum(tu, bU, ids)
    refU = F.conv_transpose2d(q, wT, bU, stride=2, padding=1).permute(0, 2, 3, 1)
    assert gotU.shape == refU.shape == (B, 2 * H, 2 * W, CU)
    assert (gotU - refU).abs().max() <= 1e-12 * refU.abs().max()
    assert not badU.any() and (magU >= gotU.abs() - 1e-9).all()


def test_bad_code_windows():
    """the pixels whose window holds a code outside [0, K): 3x3 around it for conv3, the 4x4 output block around
    (2y, 2x) clipped to the map for the transposed convolution"""
    g, w3, wT, e, b3, bU = _case(5)
    ids = torch.randint(0, K, (2, 3, 5), generator=g)
    ids[0, 1, 2] = -1
    ids[1, 0, 0] = K
    t3, tu = S.tables(w3, wT, e)
    _, _, bad3 = S.conv3_sum(t3, b3, ids)
    want3 = torch.zeros(2, 3, 5, dtype=torch.bool)
    want3[0, 0:3, 1:4] = True
    want3[1, 0:2, 0:2] = True
    assert torch.equal(bad3, want3)
    _, _, badU = S.upsample_sum(tu, bU, ids)
    wantU = torch.zeros(2, 6, 10, dtype=torch.bool)
    wantU[0, 1:5, 3:7] = True          # outputs 2y - 1 .. 2y + 2, 2x - 1 .. 2x + 2 read input (y, x)
    wantU[1, 0:3, 0:3] = True
    assert torch.equal(badU, wantU)
