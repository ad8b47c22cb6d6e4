"""rlgpu_cu_partition (host/cu_partition.cpp): the CU masks of the collection groups, checked on the host -- pairwise
disjoint, covering the device, balanced over the XCDs under both plausible bit-to-CU mappings, nested, and refused
wherever no balance can be shown (no GPU needed)."""
import numpy as np
import pytest

from rlgpu import partition
from rlgpu._lib import RLGPUError


@pytest.mark.parametrize("G", (2, 4, 8, 16))
def test_masks_are_disjoint_cover_and_balance(G):
    m = partition.masks(256, G)
    assert m.shape == (G, 8)
    bits = [set(partition.mask_bits(r)) for r in m]
    assert sum(len(b) for b in bits) == 256 and set().union(*bits) == set(range(256))
    for b in bits:
        assert [sum(k % 8 == x for k in b) for x in range(8)] == [32 // G] * 8    # bit k -> XCD k % 8
        assert [sum(k // 32 == x for k in b) for x in range(8)] == [32 // G] * 8  # 32 consecutive bits per XCD


def test_four_groups_are_the_plain_construction():
    bits = [set(partition.mask_bits(r)) for r in partition.masks(256, 4)]
    assert all(bits[g] == {k for k in range(256) if (k >> 3) % 4 == g} for g in range(4))


@pytest.mark.parametrize("G", (2, 4, 8))
def test_masks_nest(G):
    a, b = partition.masks(256, G), partition.masks(256, 2 * G)
    for g in range(G):
        np.testing.assert_array_equal(a[g], b[g] | b[g + G])


@pytest.mark.parametrize("cus,G", ((256, 0), (256, 1), (256, 3), (256, 6), (256, 32), (304, 4), (128, 2), (0, 2)))
def test_unbalanced_requests_are_refused(cus, G):
    with pytest.raises(RLGPUError):
        partition.masks(cus, G)
