"""-m gpu: the frustum packet kernel (csrc/trace_frustum.h, RSPT_CAMERA_PACKET=2: every closest-hit launch that qualifies, the trace hook
included) against the reference-order loop (RSPT_TRACE_KERNEL=0).  A sign group walks a superset of its lanes' records, decided by one
conservative test of the group's frustum per record; every lane passes the reference's own test of a leaf's box before the leaf's triangles,
so the bar is byte-identical hit records and films."""
import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.test_gpu_trace_packet import EYE, RAY_SETS, _rays, _unit, same_pixel_packets, stacked_soup
from tests.util import random_rays, small_soup

pytestmark = pytest.mark.gpu


def lens_jittered_packets(n_pixels=150, per=64, seed=23, extra=29, radius=0.05):
    """same-pixel packets whose origins are spread over a lens of `radius` around the eye: the group's o_lo / o_hi differ"""
    rays = same_pixel_packets(n_pixels, per, seed, extra)
    rng = np.random.default_rng(seed + 1)
    n = len(rays)
    r, phi = radius * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    o = np.broadcast_to(EYE, (n, 3)).copy()
    o[:, 0] += r * np.cos(phi)
    o[:, 1] += r * np.sin(phi)
    focus = EYE + rays["d"].astype(np.float64) * (3.5 / rays["d"][:, 2:3].astype(np.float64))   # the plane of focus in front of the eye (it looks along +z)
    return _rays(o, _unit(focus - o))


def short_packets(n_pixels=150, seed=31):
    """same-pixel packets whose t_max ends inside the soup, one value per packet and a few lanes shorter still: tmax_bound culls popped entries"""
    rays = same_pixel_packets(n_pixels, seed=seed, extra=11)
    rng = np.random.default_rng(seed)
    dist = float(np.linalg.norm(EYE))   # the soup sits around the origin
    per_packet = rng.uniform(dist - 0.9, dist + 0.9, len(rays) // 64 + 1)
    t = np.repeat(per_packet, 64)[: len(rays)] * rng.choice([1.0, 1.0, 1.0, 0.93], len(rays))
    rays["t_max"] = t.astype(np.float32)
    return rays


FRUSTUM_RAY_SETS = dict(RAY_SETS)
FRUSTUM_RAY_SETS["lens_jittered"] = lens_jittered_packets
FRUSTUM_RAY_SETS["t_max_inside"] = short_packets


@pytest.fixture(scope="module")
def soup(gpu):
    sc = small_soup(gpu.bvh_build)
    ds = gpu.DeviceScene(sc)
    yield sc, ds
    ds.close()


def _both(gpu, ds, rays, monkeypatch):
    monkeypatch.delenv("RSPT_CAMERA_PACKET", raising=False)
    monkeypatch.setenv("RSPT_TRACE_KERNEL", "0")
    ref = gpu.trace(ds, rays)
    monkeypatch.delenv("RSPT_TRACE_KERNEL")
    monkeypatch.setenv("RSPT_CAMERA_PACKET", "2")
    got = gpu.trace(ds, rays)
    monkeypatch.delenv("RSPT_CAMERA_PACKET")
    return got, ref


@pytest.mark.parametrize("name", sorted(FRUSTUM_RAY_SETS))
def test_frustum_hits_byte_identical_soup(gpu, soup, monkeypatch, name):
    sc, ds = soup
    rays = FRUSTUM_RAY_SETS[name]()
    got, ref = _both(gpu, ds, rays, monkeypatch)
    if name != "below_one_packet":
        assert 0 < (ref["prim"] != abi.MISS).sum()   # (the set exercises hits)
    if name in ("root_missers", "finite_t_max", "incoherent", "t_max_inside"):
        assert (ref["prim"] == abi.MISS).sum() > 0   # (... and misses)
    assert got.tobytes() == ref.tobytes()


def test_frustum_hits_byte_identical_cornell(gpu, monkeypatch):
    sc = scenes.cornell_box(gpu.bvh_build)
    with gpu.DeviceScene(sc) as ds:
        for rays in (random_rays(40037, 1, 20, 530), random_rays(20037, 2, 20, 530, t_max=300.0)):
            got, ref = _both(gpu, ds, rays, monkeypatch)
            assert got.tobytes() == ref.tobytes()


def test_frustum_big_leaves(gpu, monkeypatch):
    """leaves of 20 primitives: the gate reads the leaf's box through the big_leaves table"""
    sc = stacked_soup(gpu.bvh_build)
    assert int(np.max(sc.nodes["n_prims"])) > 15
    with gpu.DeviceScene(sc) as ds:
        for rays in (same_pixel_packets(100), lens_jittered_packets(60), random_rays(30037, 5, -1.3, 1.3)):
            got, ref = _both(gpu, ds, rays, monkeypatch)
            assert (ref["prim"] != abi.MISS).sum() > 100
            assert got.tobytes() == ref.tobytes()


def test_frustum_falls_back_where_it_cannot_serve(gpu, monkeypatch):
    """a scene whose root is a leaf, and a scene built without the leaves' boxes, keep the per-lane kernel under RSPT_CAMERA_PACKET=2"""
    sb = scenes.SceneBuilder()
    grey = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], grey, emit=(1, 1, 1))
    one_leaf = sb.finish(gpu.bvh_build)
    assert len(one_leaf.nodes) == 1
    with gpu.DeviceScene(one_leaf) as ds:
        got, ref = _both(gpu, ds, random_rays(5037, 7, -1.5, 1.5), monkeypatch)
        assert got.tobytes() == ref.tobytes()
    monkeypatch.setenv("RSPT_W4Q_BUILD", "0")
    ds = gpu.DeviceScene(small_soup(gpu.bvh_build))
    monkeypatch.delenv("RSPT_W4Q_BUILD")
    try:
        got, ref = _both(gpu, ds, same_pixel_packets(50), monkeypatch)
        assert got.tobytes() == ref.tobytes()
    finally:
        ds.close()


def _films(gpu, ds, rd, monkeypatch):
    out = []
    for v in ("0", "1", "2"):
        monkeypatch.setenv("RSPT_CAMERA_PACKET", v)
        film, _ = gpu.render(ds, rd)
        out.append(np.array(film, copy=True))
    monkeypatch.delenv("RSPT_CAMERA_PACKET")
    return out


def test_frustum_film_bit_identical_soup(gpu, soup, monkeypatch):
    sc, ds = soup
    rd = scenes.soup_render_desc(res=64, spp=64, max_depth=4)
    a, b, c = _films(gpu, ds, rd, monkeypatch)
    assert np.isfinite(a).all() and float(np.abs(a[:, :3]).sum()) > 0.0
    assert a.tobytes() == b.tobytes() == c.tobytes()


def test_frustum_film_bit_identical_cornell(gpu, monkeypatch):
    rd = scenes.cornell_render_desc(res=48, spp=64)
    with gpu.DeviceScene(scenes.cornell_box(gpu.bvh_build)) as ds:
        a, b, c = _films(gpu, ds, rd, monkeypatch)
    assert float(np.abs(a[:, :3]).sum()) > 0.0
    assert a.tobytes() == b.tobytes() == c.tobytes()
