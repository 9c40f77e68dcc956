"""-m gpu: the DEVICE's realistic camera against the REFERENCE'S OWN TEXT, with no restatement in between (beside tests/test_gpu_reference_shapes.py, which does the
same for the analytic shapes).

tests/golden/camera_functions.npz holds what the Rust text of RealisticCamera::generate_ray_differential computes (oracle/make_camera_fixtures.py compiles that text by
committed rewrite rules) for both committed prescriptions under the two descriptors of tests/test_gpu_realistic.py::test_camera_rays_hook: samples of every arm the
lens reaches, samples with p_film exactly at the film centre, within 2 ulps of an exit-pupil band border, and on the frame's last row and column.  The render
descriptor is built from the fixture's OWN element and exit-pupil tables, camera matrices, shutter and weighting — the text's tables, not the library's setup — so what
runs is the device ray function (dev_lens.h, behind rspt_camera_rays and k_raygen_lens) alone: all 22 words must be the same BITS, NaN equal to NaN.  Only the
committed file is read.

The orthographic and environment cameras have no ray hook (rspt_camera_rays refuses them: tests/test_gpu_realistic.py::test_camera_rays_hook_refusals).  Their chain
is: the text -> tests/camera_restated.cpp (tests/test_reference_camera_functions.py, on the same fixture) -> the device by per-sample radiance
(tests/test_gpu_cameras.py)."""
import numpy as np
import pytest

from tests.test_reference_camera_functions import FIXTURE, MODES, NAMES, RAY22, camera_desc, describe, unpack_camera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return np.load(FIXTURE)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_camera_rays_is_the_references_text(gpu, g, name, mode):
    key = "%s_%s" % (name, mode)
    samples, want, arm = g[name + "_samples"], g[key + "_rays"], g[name + "_arm"]
    dead, live = int((want[:, 0] == 0).sum()), int((want[:, 0] > 0).sum())
    assert dead >= 256 and live >= 512 and dead + live == len(samples) >= 900, (dead, live)      # an empty comparison cannot pass
    for a in ((0, 1, 2, 3) if name == "dgauss50" else (0, 1)):
        assert (arm == a).sum() >= 100
    rd = camera_desc(unpack_camera(g[key + "_camera"]), g[name + "_el"], g[name + "_bounds"])
    got = gpu.camera_rays(rd, samples)
    msg = describe(got, want, RAY22)
    assert msg is None, "%s: rspt_camera_rays differs from the reference's text: %s" % (key, msg)
    assert int((got[:, 0] == 0).sum()) == dead and int((got[:, 0] > 0).sum()) == live
