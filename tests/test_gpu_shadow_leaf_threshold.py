"""-m gpu: the shadow-ray kernel k_trace_w4q (csrc/trace_w4q.h) under its own leaf-phase threshold RSPT_PW_LEAF_ANY_Q.  How many parked lanes start a leaf
phase decides when a leaf's triangles are tested, never which: every flag is held byte for byte to the oracle's BVHAccel::intersect_p under RSPT_ANY_Q=1, at the
extremes of the schedule (a phase at every leaf; phases only when no lane can walk), on partial waves, through a big leaf, down a tree deeper than the LDS stack
column, with the leaf's exact box test before and after the triangles, and in a render.  (experiments/trace_w4q_deferred_leaves.patch carries the same tests for the
deferred-leaf forms of the kernel.)"""
import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.util import random_rays, small_soup

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def soup(gpu):
    sc = small_soup(gpu.bvh_build)
    ds = gpu.DeviceScene(sc)
    yield sc, ds
    ds.close()


@pytest.fixture(scope="module")
def cornell(gpu):
    sc = scenes.cornell_box(gpu.bvh_build)
    ds = gpu.DeviceScene(sc)
    yield sc, ds
    ds.close()


def ray_families(lo, hi, n=50000):
    """the four families of test_gpu_trace.test_quantised_shadow_ray_kernel_flags_are_the_references: random rays, short segments, rays with one or two zero
    direction components, rays with a huge / tiny direction"""
    rng = np.random.default_rng(606)
    sets = [random_rays(n, 61, lo, hi), random_rays(n, 62, lo, hi, t_max=0.35 * (hi - lo))]
    ax = random_rays(n, 63, lo, hi)
    k = rng.integers(0, 3, len(ax))
    d = ax["d"].copy(); d[np.arange(len(ax)), k] = 0.0; d[::3, (k[::3] + 1) % 3] = 0.0
    ax["d"] = d
    sets.append(ax)
    big = random_rays(n, 64, lo, hi)
    big["d"] = (big["d"] * np.where(rng.uniform(size=(len(big), 1)) < 0.5, 1e-25, 1e25)).astype(np.float32)
    big["d"][::2, 0] = np.float32(1.0)
    sets.append(big)
    return sets


@pytest.fixture(scope="module")
def family_refs(oracle, soup, cornell):
    """(scene, device scene, [(rays, the oracle's flags)]) for the small soup and Cornell: computed once, read by every setting"""
    out = []
    for (sc, ds), lo, hi in ((soup, -1.3, 1.3), (cornell, 20.0, 530.0)):
        out.append((sc, ds, [(rays, oracle.trace(sc, rays, any_hit=True).tobytes()) for rays in ray_families(lo, hi)]))
    return out


def set_schedule(monkeypatch, leaf):
    monkeypatch.setenv("RSPT_ANY_Q", "1")
    monkeypatch.setenv("RSPT_PW_LEAF_ANY_Q", leaf)


@pytest.mark.parametrize("leaf", ["1", "64"])
def test_extremes_of_the_schedule(gpu, family_refs, monkeypatch, leaf):
    """a leaf phase at every leaf (threshold 1) and phases only when no lane can take a node step (64)"""
    set_schedule(monkeypatch, leaf)
    for sc, ds, sets in family_refs:
        for rays, ref in sets:
            assert gpu.trace(ds, rays, any_hit=True).tobytes() == ref


@pytest.mark.parametrize("late", ["0", "1"])
def test_late_and_early_leaf_box(gpu, family_refs, monkeypatch, late):
    """the default threshold with the leaf's exact box test in front of the triangles and only behind a triangle hit"""
    monkeypatch.setenv("RSPT_ANY_Q", "1")
    monkeypatch.setenv("RSPT_ANY_Q_LATE", late)
    for sc, ds, sets in family_refs:
        for rays, ref in sets:
            assert gpu.trace(ds, rays, any_hit=True).tobytes() == ref


def test_partial_waves(gpu, oracle, soup, monkeypatch):
    """queues shorter than, equal to and just past a wave, and one past a workgroup"""
    sc, ds = soup
    all_rays = random_rays(257, 71, -1.3, 1.3, t_max=0.9)
    ref = oracle.trace(sc, all_rays, any_hit=True)
    assert 0 < (ref["prim"] == 0).sum() < len(ref)
    for leaf in ("1", "16", "64"):
        set_schedule(monkeypatch, leaf)
        for n in (1, 63, 64, 65, 257):
            assert gpu.trace(ds, all_rays[:n].copy(), any_hit=True).tobytes() == ref[:n].tobytes(), (leaf, n)


def mesh_scene(builder, P, idx):
    sb = scenes.SceneBuilder()
    sb.add_mesh(np.asarray(P, np.float32), np.asarray(idx, np.uint32), sb.add_material(scenes.matte((0.5, 0.5, 0.5))))
    return sb.finish(builder)


def segment_hits(tris, o, d):
    """(n_rays, n_tris) bool: does the segment o + t d, t in (0, 1), cross the triangle (float64 Moeller-Trumbore; the rays below keep clear of every edge)"""
    o, d = o.astype(np.float64)[:, None, :], d.astype(np.float64)[:, None, :]
    v0, e1, e2 = tris[None, :, 0].astype(np.float64), (tris[:, 1] - tris[:, 0]).astype(np.float64)[None], (tris[:, 2] - tris[:, 0]).astype(np.float64)[None]
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o - v0
        u = (s * p).sum(-1) * inv
        q = np.cross(s, e1)
        v = (d * q).sum(-1) * inv
        t = (e2 * q).sum(-1) * inv
    return (np.abs(det) > 1e-14) & (u > 0) & (v > 0) & (u + v < 1) & (t > 0) & (t < 1)


def test_big_leaf(gpu, oracle, monkeypatch):
    """40 slivers through one point whose bounds share their centre: the builder cannot split them (bvh.rs:230: centroid bounds of zero extent become a leaf), so
    that leaf has more than 16 primitives and is reached through big_leaves; 300 ordinary triangles beside it keep the root interior.  Rays aimed at a spot
    only ONE sliver covers (those of the leaf's last triangle are stopped by nothing else) and rays through the leaf's box that miss every sliver."""
    n_fan, rng = 40, np.random.default_rng(9)
    th = np.radians(10.0 + 70.0 * np.arange(n_fan) / n_fan)
    u = np.stack([np.cos(th), np.sin(th), np.zeros(n_fan)], 1)
    perp = np.stack([-np.sin(th), np.cos(th), np.zeros(n_fan)], 1)
    fan = np.stack([-u, u, 0.004 * perp], 1)                      # bounds [-|u|, |u|]: centre exactly 0 on every axis
    c = rng.uniform([3.0, -1.0, -1.0], [5.0, 1.0, 1.0], (300, 3))
    others = c[:, None, :] + rng.uniform(-0.1, 0.1, (300, 3, 3))
    P = np.concatenate([fan, others]).reshape(-1, 3).astype(np.float32)
    sc = mesh_scene(gpu.bvh_build, P, np.arange(len(P), dtype=np.uint32).reshape(-1, 3))
    leaves = np.flatnonzero(sc.nodes["n_prims"] > 16)
    assert len(leaves) == 1 and sc.nodes["n_prims"][leaves[0]] == n_fan and sc.nodes["n_prims"][0] == 0, "no big leaf under an interior root"
    first = int(sc.nodes["offset"][leaves[0]])
    leaf_tris = sc.P[sc.prims["v"][first:first + n_fan].astype(np.int64)]          # in the leaf's own order
    # a spot 0.001 inside sliver k at half its length, and the mirror spot on its bare side; the segment crosses z = 0 there, slightly tilted
    mid, side = 0.5 * (leaf_tris[:, 1] - leaf_tris[:, 0]) * 0.5, leaf_tris[:, 2] / np.linalg.norm(leaf_tris[:, 2], axis=1)[:, None]
    spots = np.concatenate([mid + 0.0005 * side, mid - 0.0005 * side, -mid + 0.0002 * side])
    spots = np.repeat(spots, 40, axis=0)
    rays = np.zeros(len(spots), abi.RAY_DT)
    tilt = rng.uniform(-0.05, 0.05, (len(spots), 2))
    d = np.concatenate([tilt, -np.ones((len(spots), 1))], 1).astype(np.float32)
    rays["d"] = d
    rays["o"] = (spots - 0.5 * d).astype(np.float32)
    rays["t_max"] = 1.0
    rays["id"] = np.arange(len(rays), dtype=np.uint32)
    hits = segment_hits(leaf_tris.astype(np.float64), rays["o"], rays["d"])
    only_last = hits[:, -1] & (hits.sum(1) == 1)
    assert only_last.sum() >= 20, "no ray is stopped by the leaf's last triangle alone"
    assert (hits.sum(1) == 0).sum() >= 1000, "no ray passes the leaf's box and misses all of it"
    ref = oracle.trace(sc, rays, any_hit=True)
    assert (ref["prim"][only_last] == 0).all() and (ref["prim"][hits.sum(1) == 0] == abi.MISS).all()
    with gpu.DeviceScene(sc) as ds:
        for leaf in ("1", "16", "64"):
            set_schedule(monkeypatch, leaf)
            assert gpu.trace(ds, rays, any_hit=True).tobytes() == ref.tobytes(), leaf


def tree_depth(nodes):
    """binary levels of a LinearBVHNode array (the first child follows its parent, `offset` is the second child)"""
    depth, todo = 0, [(0, 1)]
    while todo:
        i, lvl = todo.pop()
        depth = max(depth, lvl)
        if nodes["n_prims"][i] == 0:
            todo += [(i + 1, lvl + 1), (int(nodes["offset"][i]), lvl + 1)]
    return depth


def test_deep_stack(gpu, oracle, monkeypatch):
    """a skewed tree: 38 half-squares across the x axis at x = 13^3 .. 13^-34 (as far as normal floats go), all of one size, so every box holds the axis.  The
    builder's 12 buckets then hold one square in the last bucket and the rest in the first: every split peels ONE square off the far end, 35 binary levels (it does
    not balance this; more levels need denormal coordinates).  Rays down the axis through the bare half of the squares pass every box and hit nothing: the walk
    leaves an entry per record level and runs past the 16 stack entries a lane has in LDS into its spill rows; rays through the covered
    half are stopped."""
    n = 38
    x = (13.0 ** (3.0 - np.arange(n, dtype=np.float64))).astype(np.float32).astype(np.float64)
    assert x.min() > 1.2e-38
    tris = np.stack([np.stack([x, -np.ones(n), -np.ones(n)], 1), np.stack([x, np.ones(n), -np.ones(n)], 1), np.stack([x, -np.ones(n), np.ones(n)], 1)], 1)
    sc = mesh_scene(gpu.bvh_build, tris.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3))
    depth = tree_depth(sc.nodes)
    assert depth > 34, "the builder balanced the tree: %d binary levels" % depth
    rng = np.random.default_rng(10)
    m = 20000
    rays = np.zeros(m, abi.RAY_DT)
    y0 = np.where(np.arange(m) % 4 == 0, -0.5, 0.5) + rng.uniform(-0.05, 0.05, m)     # a quarter through the covered half (y + z < 0)
    z0 = np.where(np.arange(m) % 4 == 0, -0.5, 0.5) + rng.uniform(-0.05, 0.05, m)
    rays["o"] = np.stack([np.full(m, 4000.0), y0, z0], 1).astype(np.float32)
    off = np.where((np.arange(m) % 2 == 0)[:, None], 0.0, rng.uniform(-5e-5, 5e-5, (m, 2)))   # along the axis, and slightly off it (0.2 over the whole length)
    sign = np.where(np.arange(m) % 8 < 6, -1.0, 1.0)                                 # (some look away from beyond the far end: the root's box fails)
    rays["d"] = np.concatenate([sign[:, None], off], 1).astype(np.float32)
    rays["t_max"] = np.where(np.arange(m) % 16 == 5, 3000.0, np.inf)                 # (some stop between the first two squares)
    rays["id"] = np.arange(m, dtype=np.uint32)
    ref = oracle.trace(sc, rays, any_hit=True)
    assert 2000 < (ref["prim"] == 0).sum() < m - 8000      # (the oracle runs on the CPU)
    with gpu.DeviceScene(sc) as ds:
        for leaf in ("1", "16", "64"):
            set_schedule(monkeypatch, leaf)
            assert gpu.trace(ds, rays, any_hit=True).tobytes() == ref.tobytes(), leaf


def test_render_with_the_quantised_kernel_forced(gpu, cornell, monkeypatch):
    """the Cornell frame of test_gpu_render at its smallest size: per-sample radiance with k_trace_w4q forced, at either extreme and the default threshold, equals
    the plain shadow-ray kernel's"""
    sc, ds = cornell
    rd = scenes.cornell_render_desc(res=32, spp=8)
    monkeypatch.setenv("RSPT_ANY_Q", "0")
    plain = gpu.render_samples(ds, rd)[0]
    for leaf in ("1", "16", "64"):
        set_schedule(monkeypatch, leaf)
        assert np.array_equal(gpu.render_samples(ds, rd)[0], plain), leaf
