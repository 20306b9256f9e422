"""Choice of the serving coalescing factor (no GPU needed)."""

import pytest

from roko_amd.ops.forward import coalesce_width


@pytest.mark.parametrize("request_,depth,want", [
    # depth 48 = 16 * 3 allows 1, 2, 4, 8, 16
    (1, 48, 1), (2, 48, 2), (3, 48, 2), (4, 48, 4), (7, 48, 4), (8, 48, 8),
    (16, 48, 16), (32, 48, 16), (1000, 48, 16),
    # odd depths never coalesce
    (4, 3, 1), (4, 1, 1), (16, 1, 1), (8, 9, 1),
    # the power of two must divide depth
    (8, 4, 4), (8, 12, 4), (4, 6, 2), (8, 8, 8), (16, 32, 16), (64, 32, 32),
    # nonsense requests fall back to 1
    (0, 48, 1), (-3, 48, 1),
])
def test_coalesce_width(request_, depth, want):
    g = coalesce_width(request_, depth)
    assert g == want
    assert depth % g == 0 and g & (g - 1) == 0
