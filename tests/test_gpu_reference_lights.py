"""-m gpu: the projection and goniometric lights on the DEVICE held to the reference's own text (tests/golden/light_functions.npz, written by
oracle/make_light_fixtures.py; this file reads nothing outside the repository tree).

Tables.  rspt_light_distribution is the device's hook for these lights: k_ld_fixed_ml runs light_power, k_ld_contrib_ml runs light_sample_li at the 128 points of every
voxel without a visibility test, which is SpatialLightDistribution::compute_distribution.  On both committed scenes and under all three strategies func, cdf, nvox and
the voxel equal the TEXT's tables bit for bit at every committed point: no restatement sits in between.  The committed voxels' sample points reach every class of both
lights (behind the hither plane, beyond each of the four edges, inside, each phi quadrant: counted by the generator, checked in tests/test_reference_light_functions.py).

Edge rooms.  A depth-1 path render of one floor under (a) a projector whose image rectangle lies wholly inside the frame, (b) a goniometric light whose pole and seam
fall on the floor, per camera sample against tests/maplight_restated.cpp, which tests/test_reference_light_functions.py holds to the text word for word."""
import numpy as np
import pytest

from rs_pbrt_amd import abi
from tests.test_maplight_host import assert_same_li, restated_render
from tests.test_reference_light_functions import EDGE_CLASSES, FIXTURE, N_SCENES, STRATEGIES, edge_classes, edge_rd, edge_room, restated_lib, same_bits, table_scene
from tests.util import shade_instantiation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return dict(np.load(FIXTURE))


@pytest.fixture(scope="module")
def restated():
    return restated_lib()


@pytest.mark.parametrize("k", range(N_SCENES))
def test_light_tables_equal_the_references_text(gpu, g, k):
    sc = table_scene(gpu.bvh_build, g, k)
    kinds = list(sc.lights["kind"])
    assert kinds.count(abi.LIGHT_PROJECTION) == 3 and kinds.count(abi.LIGHT_GONIOMETRIC) == 3 and kinds.count(abi.LIGHT_DIFFUSE_AREA) == 1 and kinds.count(abi.LIGHT_POINT) == 1
    pts = g["tab%d_pts" % k]
    bad = []
    with gpu.DeviceScene(sc) as ds:
        for name, strategy in STRATEGIES:
            key = "tab%d_%s" % (k, name)
            differing = 0
            for i, p in enumerate(pts):
                func, cdf, nvox, voxel = gpu.light_distribution(ds, strategy, p)
                ok = list(nvox) == list(g[key + "_nvox"]) and list(voxel) == list(g[key + "_voxel"][i]) and same_bits(func, g[key + "_func"][i]).all() and same_bits(cdf, g[key + "_cdf"][i]).all()
                differing += not ok
            if differing:
                bad.append("%s: %d of %d points differ from the text's table" % (key, differing, len(pts)))
            print("%s: %d points, %d lights, grid %s, %d differ" % (key, len(pts), len(kinds), list(g[key + "_nvox"]), differing))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("which", ["projector", "goniometric"])
def test_edge_room_li_equals_restated_li(gpu, restated, monkeypatch, capfd, which, sampler):
    from oracle import pyoracle      # (the checker: first hits on the CPU)
    pyoracle.build()
    sc = edge_room(gpu.bvh_build, which)
    rd = edge_rd(sampler)
    n, counts = edge_classes(restated, pyoracle, sc, rd, which)
    assert all(c >= 32 for c in counts), dict(zip(EDGE_CLASSES[which], counts))

    def render():
        with gpu.DeviceScene(sc) as ds:
            return gpu.render_samples(ds, rd)[0]
    li, name = shade_instantiation(monkeypatch, capfd, render)
    assert name == "generic-maplight"
    want = restated_render(restated, sc, rd)[1]
    print("%s %s: %d first hits, classes %s, %d camera samples, mean %.4f, dark share %.3f" % (which, sampler, n, dict(zip(EDGE_CLASSES[which], counts)), li.shape[0] * li.shape[1], np.nanmean(li), (li.max(axis=-1) == 0).mean()))
    assert_same_li(li, want)
    assert np.nanmean(li) > 0.0 and (li.max(axis=-1) == 0).mean() > 0.05      # lit and dark samples both
