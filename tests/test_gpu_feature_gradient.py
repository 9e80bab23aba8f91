"""k_gradient_image (camera_calibration_amd/csrc/kernels_features.hip) against numpy: every float equal (differences of bytes divided
by 1 or 2 are exact in float32)."""
import numpy as np
import pytest

import feature_refinement_reference as ref
from camera_calibration_amd import feature_refinement as fr

pytestmark = pytest.mark.gpu


def _images(width, height):
    yy, xx = np.mgrid[0:height, 0:width]
    return dict(constant=np.full((height, width), 77, np.uint8), ramp=((3 * xx + 5 * yy) % 256).astype(np.uint8),
                random=np.random.default_rng(width * 1000 + height).integers(0, 256, (height, width)).astype(np.uint8),
                extremes=np.where((xx + yy) % 2 == 0, 0, 255).astype(np.uint8))


@pytest.mark.parametrize("width,height", [(2, 2), (2, 65), (65, 2), (97, 63)])      # one pixel tile and ragged tiles in x and in y
def test_gradient_image_equals_numpy(width, height):
    r = fr.FeatureRefiner(width, height, 1, fr.GRADIENTS_XY, fr.make_samples(1))
    try:
        for name, image in _images(width, height).items():
            r.set_image(image)
            got, want = r.gradient(), ref.gradient_image(image)
            assert got.shape == want.shape == (height, width, 2)
            assert np.array_equal(got, want), name
            if name == "constant":
                assert not got.any()
    finally:
        r.close()
