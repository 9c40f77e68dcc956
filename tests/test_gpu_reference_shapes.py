"""-m gpu: the DEVICE's sphere, disk and cylinder intersection against the REFERENCE'S OWN TEXT, with no restatement in between (beside
tests/test_gpu_reference_geometry.py, which does the same for the triangle side).

tests/golden/shape_functions.npz holds what the Rust text of Sphere / Disk / Cylinder::intersect and intersect_p computes on at least 2^11 seeded cases per shape
(oracle/make_shape_fixtures.py compiles that text by committed rewrite rules): rays from outside and inside, first roots clipped away, origins spawned on the
surface, t_max at the text's own t and at its upper bound, grazing and plane-parallel rays, azimuths at 0 / phi_max / 2 pi, a disk's centre and rims, records with the
orientation flags set.  rspt_quadric_intersect (dev_sphere.h sphere_hit, dev_quadric.h disk_hit / cylinder_hit / quadric_to_world) and, for spheres,
rspt_libm(RSPT_LIBM_SPHERE) run over the same elements: all 64 output words must be the same BITS.  Only the committed file is read."""
import numpy as np
import pytest

from rs_pbrt_amd import abi
from tests.test_quadric_host import SHAPES
from tests.test_reference_shape_functions import FIXTURE, SHAPE_NAMES, describe, fixture_elements

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return np.load(FIXTURE)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_quadric_intersect_is_the_references_text(gpu, g, shape):
    x, want = fixture_elements(g, shape)
    n, hits = len(x), int(want[:, 0].sum())
    assert n >= 1 << 11 and hits * 4 >= n and (n - hits) * 4 >= n, (shape, n, hits)      # at least a quarter hits and a quarter misses by the text
    out = np.zeros_like(x)
    assert gpu.lib().rspt_quadric_intersect(SHAPES[shape], x.ctypes.data, n, out.ctypes.data) == 0, gpu.lib().rspt_last_error()
    msg = describe(out, want)
    assert msg is None, "%s: rspt_quadric_intersect differs from the reference's text: %s" % (shape, msg)


def test_libm_sphere_is_the_references_text(gpu, g):
    x, want = fixture_elements(g, "sphere")
    out = np.zeros_like(x)
    assert gpu.lib().rspt_libm(abi.LIBM_SPHERE, x.ctypes.data, None, len(x), out.ctypes.data) == 0, gpu.lib().rspt_last_error()
    msg = describe(out, want)
    assert msg is None, "RSPT_LIBM_SPHERE differs from the reference's text: %s" % msg
