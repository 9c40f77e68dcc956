"""-m gpu: the bundle kernels (csrc/trace_bundle.h, RSPT_CAMERA_PACKET=3 / 4: one frustum walk per bundle of two / four packets, for every closest-hit
launch that qualifies, the trace hook included) against the reference-order loop (RSPT_TRACE_KERNEL=0).  A bundle walks a superset of its rays' records and
every ray passes the reference's own test of a leaf's box before the leaf's triangles; a bundle that does not qualify is served packet by packet by the code
of the frustum packet kernel.  The bar is byte-identical hit records and films."""
import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.test_gpu_trace_frustum import FRUSTUM_RAY_SETS, lens_jittered_packets
from tests.test_gpu_trace_packet import EYE, RENDERS, _rays, _unit, same_pixel_packets, stacked_soup
from tests.util import random_rays, small_soup

pytestmark = pytest.mark.gpu

MODES = {"3": 2, "4": 4}   # RSPT_CAMERA_PACKET -> packets per bundle
HALF = np.tan(np.radians(scenes.SOUP_FOV) / 2)
PIXEL = 2 * HALF / 1024


def _pixels_to_rays(centres, per, seed):
    """`per` jittered rays through each pixel (its corner given in image-plane units), in queue order"""
    rng = np.random.default_rng(seed)
    px = np.repeat(np.asarray(centres, np.float64), per, axis=0)
    px = px + rng.uniform(0, PIXEL, px.shape)
    return _rays(EYE, _unit(np.concatenate([px, np.ones((len(px), 1))], axis=1)))


def whole_pixel_bundles():
    """256 samples per pixel: a bundle of two or four packets is one pixel"""
    return same_pixel_packets(n_pixels=60, per=256)


def distant_pixel_bundles():
    """every packet another, distant pixel: a bundle's hull is wide (or its packets differ in their signs)"""
    return same_pixel_packets(n_pixels=240, per=64, seed=41, extra=5)


def axis_plane_bundles(seed=43):
    """bundles of one pixel on the image's centre column and centre row (the jitter straddles 0: two sign groups, four at the centre, with lanes in every set);
    a few directions of every third pixel have a component of exactly +0 or -0: a literal-chain ray inside an otherwise narrow bundle"""
    rng = np.random.default_rng(seed)
    along = rng.uniform(-0.4, 0.4, 20) * HALF
    centres = [(-PIXEL / 2, v) for v in along] + [(v, -PIXEL / 2) for v in along] + [(-PIXEL / 2, -PIXEL / 2)] * 2
    rays = _pixels_to_rays(centres, 256, seed)
    d = rays["d"]
    for p in range(0, len(centres), 3):
        axis = 0 if p < 20 or p >= 40 else 1
        for k in rng.integers(0, 256, 3):
            d[p * 256 + k, axis] = 0.0 if k & 1 else -0.0
    rays["d"] = _unit(d.astype(np.float64)).astype(np.float32)
    return rays


def one_empty_set_bundles(seed=47):
    """whole-pixel bundles in which one whole packet looks away from the scene (it misses the root's box) while the others hit"""
    rays = same_pixel_packets(n_pixels=48, per=256, seed=seed, extra=0)
    d = rays["d"].reshape(48, 4, 64, 3)
    for p in range(48):
        d[p, p % 4] *= -1.0
    rays["d"] = d.reshape(-1, 3)
    return rays


def shrinking_t_max_bundles(seed=53):
    """whole-pixel bundles with one t_max per packet, inside the soup: the sets of one bundle have very different t_max"""
    rays = same_pixel_packets(n_pixels=60, per=256, seed=seed, extra=19)
    rng = np.random.default_rng(seed)
    dist = float(np.linalg.norm(EYE))   # the soup sits around the origin
    per_packet = rng.uniform(dist - 0.95, dist + 0.95, len(rays) // 64 + 1)
    rays["t_max"] = np.repeat(per_packet, 64)[: len(rays)].astype(np.float32)
    return rays


BUNDLE_RAY_SETS = dict(FRUSTUM_RAY_SETS)
BUNDLE_RAY_SETS.update(whole_pixel=whole_pixel_bundles, distant_pixels=distant_pixel_bundles, axis_plane=axis_plane_bundles, one_empty_set=one_empty_set_bundles,
                       shrinking_t_max=shrinking_t_max_bundles)
WITH_MISSES = ("root_missers", "finite_t_max", "incoherent", "t_max_inside", "one_empty_set", "shrinking_t_max")


@pytest.fixture(scope="module")
def soup(gpu):
    sc = small_soup(gpu.bvh_build)
    ds = gpu.DeviceScene(sc)
    yield sc, ds
    ds.close()


def _reference(gpu, ds, rays, monkeypatch):
    monkeypatch.delenv("RSPT_CAMERA_PACKET", raising=False)
    monkeypatch.setenv("RSPT_TRACE_KERNEL", "0")
    ref = gpu.trace(ds, rays)
    monkeypatch.delenv("RSPT_TRACE_KERNEL")
    return ref


def _bundled(gpu, ds, rays, monkeypatch, mode):
    monkeypatch.setenv("RSPT_CAMERA_PACKET", mode)
    got = gpu.trace(ds, rays)
    monkeypatch.delenv("RSPT_CAMERA_PACKET")
    return got


_soup_refs = {}   # ray set -> (rays, the reference-order kernel's records): computed once, shared by both bundle sizes


def _soup_case(gpu, ds, monkeypatch, name):
    if name not in _soup_refs:
        rays = BUNDLE_RAY_SETS[name]()
        ref = _reference(gpu, ds, rays, monkeypatch)
        ref.setflags(write=False)
        _soup_refs[name] = (rays, ref)
    return _soup_refs[name]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(BUNDLE_RAY_SETS))
def test_bundle_hits_byte_identical_soup(gpu, soup, monkeypatch, name, mode):
    sc, ds = soup
    rays, ref = _soup_case(gpu, ds, monkeypatch, name)
    if name != "below_one_packet":
        assert 0 < (ref["prim"] != abi.MISS).sum()   # (the set exercises hits)
    if name in WITH_MISSES:
        assert (ref["prim"] == abi.MISS).sum() > 0   # (... and misses)
    if name == "one_empty_set":
        away = rays["d"][:, 2] < 0
        assert away.sum() == 48 * 64 and (ref["prim"][away] == abi.MISS).all() and (ref["prim"][~away] != abi.MISS).sum() > 0
    if name == "axis_plane":
        assert (rays["d"] == 0).sum() > 0 and (rays["d"][:, 0] < 0).sum() > 1000 and (rays["d"][:, 0] > 0).sum() > 1000
    got = _bundled(gpu, ds, rays, monkeypatch, mode)
    assert got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_bundle_ray_counts_around_the_bundle_size(gpu, soup, monkeypatch, mode):
    """the queue's tail: a last bundle with one ray, with one packet short of a ray, with exactly one packet, one packet and a ray, and one ray in its last set"""
    sc, ds = soup
    r = MODES[mode]
    rays, ref = _soup_case(gpu, ds, monkeypatch, "whole_pixel")
    for k in (0, 1, 3):
        for tail in (1, 63, 64, 65, 64 * (r - 1) + 1):
            n = 64 * r * k + tail
            got = _bundled(gpu, ds, rays[:n].copy(), monkeypatch, mode)
            assert got.tobytes() == ref[:n].tobytes(), (k, tail)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_bundle_hits_byte_identical_cornell(gpu, monkeypatch, mode):
    sc = scenes.cornell_box(gpu.bvh_build)
    with gpu.DeviceScene(sc) as ds:
        for rays in (random_rays(40037, 1, 20, 530), random_rays(20037, 2, 20, 530, t_max=300.0)):
            ref = _reference(gpu, ds, rays, monkeypatch)
            assert _bundled(gpu, ds, rays, monkeypatch, mode).tobytes() == ref.tobytes()


def test_bundle_big_leaves(gpu, monkeypatch):
    """leaves of 20 primitives: the gate reads the leaf's box through the big_leaves table, and every set runs the leaf's twenty triangles"""
    sc = stacked_soup(gpu.bvh_build)
    assert int(np.max(sc.nodes["n_prims"])) > 15
    with gpu.DeviceScene(sc) as ds:
        for rays in (same_pixel_packets(40, per=256), lens_jittered_packets(60), random_rays(30037, 5, -1.3, 1.3)):
            ref = _reference(gpu, ds, rays, monkeypatch)
            assert (ref["prim"] != abi.MISS).sum() > 100
            for mode in sorted(MODES):
                assert _bundled(gpu, ds, rays, monkeypatch, mode).tobytes() == ref.tobytes(), mode


def test_bundle_falls_back_where_it_cannot_serve(gpu, monkeypatch):
    """a scene whose root is a leaf, and a scene built without the leaves' boxes, keep the per-lane kernel under RSPT_CAMERA_PACKET=3 / 4"""
    sb = scenes.SceneBuilder()
    grey = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], grey, emit=(1, 1, 1))
    one_leaf = sb.finish(gpu.bvh_build)
    assert len(one_leaf.nodes) == 1
    with gpu.DeviceScene(one_leaf) as ds:
        rays = random_rays(5037, 7, -1.5, 1.5)
        ref = _reference(gpu, ds, rays, monkeypatch)
        for mode in sorted(MODES):
            assert _bundled(gpu, ds, rays, monkeypatch, mode).tobytes() == ref.tobytes(), mode
    monkeypatch.setenv("RSPT_W4Q_BUILD", "0")
    ds = gpu.DeviceScene(small_soup(gpu.bvh_build))
    monkeypatch.delenv("RSPT_W4Q_BUILD")
    try:
        rays = same_pixel_packets(20, per=256)
        ref = _reference(gpu, ds, rays, monkeypatch)
        for mode in sorted(MODES):
            assert _bundled(gpu, ds, rays, monkeypatch, mode).tobytes() == ref.tobytes(), mode
    finally:
        ds.close()


def _films(gpu, ds, rd, monkeypatch):
    out = []
    for v in ("0", "2", "3", "4"):
        monkeypatch.setenv("RSPT_CAMERA_PACKET", v)
        film, _ = gpu.render(ds, rd)
        out.append(np.array(film, copy=True))
    monkeypatch.delenv("RSPT_CAMERA_PACKET")
    return out


BUNDLE_RENDERS = {
    "one_pixel_per_bundle": dict(res=32, spp=256),
    "four_pixels_per_bundle": dict(res=64, spp=64),
    "crop_partial_bundles": RENDERS["crop_partial_packets"],
    "shard": RENDERS["shard"],
    "lens": RENDERS["lens"],
    "moving_camera": RENDERS["moving_camera"],
}


@pytest.mark.parametrize("name", sorted(BUNDLE_RENDERS))
def test_bundle_films_bit_identical_soup(gpu, soup, monkeypatch, name):
    sc, ds = soup
    kw = dict(BUNDLE_RENDERS[name])
    rd = scenes.soup_render_desc(res=kw.pop("res"), spp=kw.pop("spp"), max_depth=4, **kw)
    films = _films(gpu, ds, rd, monkeypatch)
    assert np.isfinite(films[0]).all() and float(np.abs(films[0][:, :3]).sum()) > 0.0
    for f in films[1:]:
        assert f.tobytes() == films[0].tobytes()


def test_bundle_film_bit_identical_cornell(gpu, monkeypatch):
    rd = scenes.cornell_render_desc(res=48, spp=64)
    with gpu.DeviceScene(scenes.cornell_box(gpu.bvh_build)) as ds:
        films = _films(gpu, ds, rd, monkeypatch)
    assert float(np.abs(films[0][:, :3]).sum()) > 0.0
    for f in films[1:]:
        assert f.tobytes() == films[0].tobytes()
