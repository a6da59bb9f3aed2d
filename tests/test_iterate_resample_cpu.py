"""CPU: the premises of tests/test_iterate_resample_gpu.py at pyr_scale 0.501 and 0.499 -- a 272 x 400 frame keeps the
level sizes of pyr_scale 0.5, every level the exact double of the next (so the driver takes the resampling first
iteration), and the factor float(1 / pyr_scale) that iteration multiplies by is not a power of two (so the place of that
product in the blend shows in the bits)."""
import numpy as np
import pytest

OTHER_SCALES = (0.501, 0.499)


@pytest.mark.parametrize("pyr_scale", OTHER_SCALES)
def test_level_sizes_are_those_of_one_half(nsof_lib, pyr_scale):
    h, w = 272, 400
    assert nsof_lib.effective_levels(w, h, pyr_scale, 3) == 3
    sizes = [nsof_lib.level_size(w, h, pyr_scale, k)[:2] for k in range(4)]
    assert sizes == [(400, 272), (200, 136), (100, 68), (50, 34)], sizes
    assert sizes == [nsof_lib.level_size(w, h, 0.5, k)[:2] for k in range(4)]


@pytest.mark.parametrize("pyr_scale", OTHER_SCALES)
def test_factor_is_not_a_power_of_two(pyr_scale):
    mul = np.float32(1.0 / pyr_scale)
    assert np.isfinite(mul) and 1.9 < mul < 2.1
    assert int(mul.view(np.uint32)) & 0x007FFFFF != 0, hex(int(mul.view(np.uint32)))
    assert int(np.float32(1.0 / 0.5).view(np.uint32)) & 0x007FFFFF == 0      # the factor the suite ran with so far
    # so the product is inexact: there are float32 values whose product with it needs rounding
    x = np.float32(1.0) + np.float32(2.0 ** -23)
    assert np.float64(x) * np.float64(mul) != np.float64(x * mul)
