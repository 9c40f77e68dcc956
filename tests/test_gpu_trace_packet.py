"""-m gpu: the packet traversal kernel (csrc/trace_packet.h, RSPT_CAMERA_PACKET=1: every closest-hit launch that qualifies, the trace hook
included) against the reference-order loop (RSPT_TRACE_KERNEL=0).  One stack per wave, records and triangles fetched once per wave — every lane
still runs its own reference test sequence, so the bar is byte-identical hit records and films."""
import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.util import random_rays, small_soup

pytestmark = pytest.mark.gpu

EYE = np.array(scenes.SOUP_LOOK_AT[0], np.float64)


def _rays(o, d, t_max=np.inf):
    n = len(d)
    rays = np.zeros(n, abi.RAY_DT)
    rays["o"] = np.broadcast_to(np.asarray(o, np.float64), (n, 3)).astype(np.float32)
    rays["d"] = np.asarray(d, np.float64).astype(np.float32)
    rays["t_max"] = t_max
    rays["id"] = np.arange(n, dtype=np.uint32)
    return rays


def _unit(d):
    return d / np.linalg.norm(d, axis=1)[:, None]


def same_pixel_packets(n_pixels=200, per=64, seed=5, extra=37):
    """64 jittered rays through each of n_pixels pixels of a 1024-wide frame of the soup (what a wave of the camera launch holds), and `extra` more so that
    the last packet is a partial one"""
    rng = np.random.default_rng(seed)
    half = np.tan(np.radians(scenes.SOUP_FOV) / 2)
    px = rng.uniform(-0.45, 0.45, (n_pixels + 1, 2)) * half
    px = np.repeat(px, per, axis=0)[: n_pixels * per + extra]
    px += rng.uniform(0, 2 * half / 1024, px.shape)
    return _rays(EYE, _unit(np.concatenate([px, np.ones((len(px), 1))], axis=1)))


def pixel_grid(res=128):
    half = np.tan(np.radians(scenes.SOUP_FOV) / 2)
    g = (np.arange(res) + 0.5) / res * 2 - 1
    x, y = np.meshgrid(g * half, g * half)
    return _rays(EYE, _unit(np.stack([x.ravel(), y.ravel(), np.ones(res * res)], axis=1)))


def mixed_octants(n=20037, seed=9):
    """lane k of every packet looks into octant k % 8: eight sign groups per packet"""
    rng = np.random.default_rng(seed)
    d = np.abs(rng.normal(size=(n, 3))) + 1e-3
    k = np.arange(n)
    d *= np.stack([1 - 2 * (k & 1), 1 - 2 * ((k >> 1) & 1), 1 - 2 * ((k >> 2) & 1)], axis=1)
    return _rays(rng.uniform(-0.4, 0.4, (n, 3)), _unit(d))


def axis_and_zero_components(n=12037, seed=11):
    """axis-parallel directions and directions with one or two zero (+0 and -0) components, mixed into packets with ordinary ones"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    kind = rng.integers(0, 4, n)
    for axis in range(3):
        zero = (kind == 1) & (rng.integers(0, 3, n) == axis) | (kind == 2) & (rng.integers(0, 3, n) != axis)
        d[zero, axis] = np.where(rng.integers(0, 2, zero.sum()) == 0, 0.0, -0.0)
    d[np.abs(d).sum(axis=1) == 0] = (0.0, -1.0, 0.0)
    return _rays(rng.uniform(-1.1, 1.1, (n, 3)), _unit(d))


def root_missers(n=8037, seed=13):
    """half of the lanes start outside the scene's bounds and look away from it"""
    rng = np.random.default_rng(seed)
    rays = random_rays(n, seed, -1.2, 1.2)
    away = rng.integers(0, 2, n) == 1
    o = rng.uniform(3.0, 4.0, (n, 3)) * np.where(rng.integers(0, 2, (n, 3)) == 0, -1.0, 1.0)
    rays["o"][away] = o[away].astype(np.float32)
    rays["d"][away] = _unit(o[away]).astype(np.float32)
    return rays


def stacked_soup(builder, n=3000, stacks=60, copies=20, seed=21):
    """a soup in which `stacks` triangles come `copies` times each, with one centroid: the builder cannot split them, so they share a leaf of 20 primitives"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    tri = (c + rng.uniform(-0.06, 0.06, (n, 3, 3))).astype(np.float32)
    tri = np.concatenate([tri, np.repeat(tri[:stacks], copies - 1, axis=0)])
    sb = scenes.SceneBuilder()
    grey = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_mesh(tri.reshape(-1, 3), np.arange(3 * len(tri), dtype=np.uint32).reshape(-1, 3), grey)
    sb.add_quad([(0.5, 1.5, -0.5), (0.5, 1.5, 0.5), (-0.5, 1.5, 0.5), (-0.5, 1.5, -0.5)], grey, emit=(40, 40, 40))
    return sb.finish(builder)


RAY_SETS = {
    "same_pixel": same_pixel_packets,
    "pixel_grid": pixel_grid,
    "incoherent": lambda: random_rays(50037, 3, -1.3, 1.3),
    "mixed_octants": mixed_octants,
    "axis_and_zero": axis_and_zero_components,
    "finite_t_max": lambda: random_rays(30037, 17, -1.2, 1.2, t_max=np.random.default_rng(17).uniform(0.02, 1.5, 30037).astype(np.float32)),
    "root_missers": root_missers,
    "below_one_packet": lambda: same_pixel_packets(n_pixels=0, extra=37),
}


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
    monkeypatch.setenv("RSPT_CAMERA_PACKET", "1")
    got = gpu.trace(ds, rays)
    monkeypatch.delenv("RSPT_CAMERA_PACKET")
    return got, ref


@pytest.mark.parametrize("name", sorted(RAY_SETS))
def test_packet_hits_byte_identical_soup(gpu, soup, monkeypatch, name):
    sc, ds = soup
    rays = RAY_SETS[name]()
    got, ref = _both(gpu, ds, rays, monkeypatch)
    if name != "below_one_packet":
        assert 0 < (ref["prim"] != abi.MISS).sum()   # (the set exercises hits)
    if name in ("root_missers", "finite_t_max", "incoherent"):
        assert (ref["prim"] == abi.MISS).sum() > 0   # (... and misses)
    assert got.tobytes() == ref.tobytes()


def test_packet_hits_byte_identical_cornell(gpu, monkeypatch):
    sc = scenes.cornell_box(gpu.bvh_build)
    with gpu.DeviceScene(sc) as ds:
        for rays in (random_rays(40037, 1, 20, 530), random_rays(20037, 2, 20, 530, t_max=300.0)):
            got, ref = _both(gpu, ds, rays, monkeypatch)
            assert got.tobytes() == ref.tobytes()


def test_packet_big_leaves(gpu, monkeypatch):
    """leaves of more than 15 primitives go through the big_leaves table"""
    sc = stacked_soup(gpu.bvh_build)
    assert int(np.max(sc.nodes["n_prims"])) > 15
    with gpu.DeviceScene(sc) as ds:
        for rays in (same_pixel_packets(100), random_rays(30037, 5, -1.3, 1.3)):
            got, ref = _both(gpu, ds, rays, monkeypatch)
            assert (ref["prim"] != abi.MISS).sum() > 100
            assert got.tobytes() == ref.tobytes()


def test_packet_falls_back_where_it_cannot_serve(gpu, monkeypatch):
    """a scene whose root is a leaf, and a scene built without the leaves' boxes, keep the per-lane kernel under RSPT_CAMERA_PACKET=1"""
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
    for v in ("0", "1"):
        monkeypatch.setenv("RSPT_CAMERA_PACKET", v)
        film, _ = gpu.render(ds, rd)
        out.append(np.array(film, copy=True))
    monkeypatch.delenv("RSPT_CAMERA_PACKET")
    return out


RENDERS = {
    "plain": dict(res=48, spp=64),
    "lens": dict(res=40, spp=64, lens_radius=0.05, focal_distance=3.5),
    "moving_camera": dict(res=40, spp=64, look_at_end=((0.3, 0.1, -4), (0, 0, 0), (0, 1, 0))),
    "halton": dict(res=40, spp=64, sampler="halton"),
    "crop_partial_packets": dict(res=50, spp=8, crop=(0.1, 0.63, 0.2, 0.77)),
    "shard": dict(res=50, spp=8, shard=(1, 3, 1)),
}


@pytest.mark.parametrize("name", sorted(RENDERS))
def test_packet_films_bit_identical_soup(gpu, soup, monkeypatch, name):
    sc, ds = soup
    kw = dict(RENDERS[name])
    rd = scenes.soup_render_desc(res=kw.pop("res"), spp=kw.pop("spp"), max_depth=4, **kw)
    a, b = _films(gpu, ds, rd, monkeypatch)
    assert np.isfinite(a).all() and float(np.abs(a[:, :3]).sum()) > 0.0
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["plain", "lens", "halton"])
def test_packet_films_bit_identical_cornell(gpu, monkeypatch, name):
    kw = dict(RENDERS[name])
    kw.pop("focal_distance", None)
    if "lens_radius" in kw:
        kw.update(lens_radius=8.0, focal_distance=900.0)
    rd = scenes.cornell_render_desc(res=kw.pop("res"), spp=kw.pop("spp"), **kw)
    with gpu.DeviceScene(scenes.cornell_box(gpu.bvh_build)) as ds:
        a, b = _films(gpu, ds, rd, monkeypatch)
    assert float(np.abs(a[:, :3]).sum()) > 0.0
    assert a.tobytes() == b.tobytes()
