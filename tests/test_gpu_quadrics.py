"""-m gpu: disks and cylinders (ABI 27) on the device — rspt_quadric_intersect and the quadric traversal of rspt_trace, bit for bit against a hand
restatement of Disk::intersect / Cylinder::intersect with transform_surface_interaction (tests/quadric_restated.cpp, compiled here with g++ and the
host libm; tests/test_quadric_host.py holds it to closed-form answers), and every refusal of rspt_scene_create."""
import ctypes as C
import re
import sys

import numpy as np
import pytest

from rs_pbrt_amd import abi, scenes
from tests.test_quadric_host import HIT, HIT_P, SHAPES, build_quadric_restated, directed_cases, hook_cases, pack, restated_hook
from tests.util import xf

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ref():
    return build_quadric_restated()


def device_hook(gpu, shape, x):
    x = np.ascontiguousarray(np.atleast_2d(x), F32)
    out = np.zeros_like(x)
    rc = gpu.lib().rspt_quadric_intersect(SHAPES[shape], x.ctypes.data, len(x), out.ctypes.data)
    assert rc == 0, gpu.lib().rspt_last_error()
    return out


def assert_same_bits(got, want):
    bad = np.nonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[0], :25], want[bad[0], :25])


@pytest.mark.parametrize("shape", ["disk", "cylinder", "sphere"])
def test_hook_bit_exact(gpu, ref, shape):
    """all 64 outputs (the 44 that are used and the zeros around them) of 2^14 random cases, at least a quarter hits and a quarter misses by the restatement"""
    n = 1 << 14
    x = hook_cases(shape, n)
    want = restated_hook(ref, shape, x)
    hits = int(want[:, HIT].sum())
    assert hits >= n // 4 and n - hits >= n // 4, (hits, n)
    assert np.array_equal(want[:, HIT], want[:, HIT_P])
    assert_same_bits(device_hook(gpu, shape, x), want)


def test_hook_directed_edge_cases(gpu, ref):
    """the closed-form cases of tests/test_quadric_host.py, and t_max at / one ulp behind a disk's t"""
    for name, case in directed_cases().items():
        shape, rec, o, d, t_max, expect = case
        x = [pack(rec, o, d, t_max)]
        t = restated_hook(ref, shape, x[0])[0][1]
        if expect:
            x += [pack(rec, o, d, t), pack(rec, o, d, np.nextafter(t, F32(np.inf))), pack(rec, o, d, np.nextafter(t, F32(0)))]
        x = np.array(x)
        want = restated_hook(ref, shape, x)
        got = device_hook(gpu, shape, x)
        assert bool(got[0, HIT]) == expect and bool(got[0, HIT_P]) == expect, name
        assert_same_bits(got, want)
        if expect and shape == "disk":
            assert got[1, HIT] == 0 and got[2, HIT] == 1 and got[3, HIT] == 0, name


def test_hook_with_mesh_sphere_is_the_libm_sphere_hook(gpu):
    n = 4096
    x = hook_cases("sphere", n)
    want = np.zeros_like(x)
    assert gpu.lib().rspt_libm(abi.LIBM_SPHERE, x.ctypes.data, None, n, want.ctypes.data) == 0, gpu.lib().rspt_last_error()
    assert want[:, HIT].sum() > n // 4
    assert_same_bits(device_hook(gpu, "sphere", x), want)
    rec = np.frombuffer(x[:8, :42].tobytes(), abi.SPHERE_DT)
    assert np.array_equal(gpu.quadric_intersect(abi.MESH_SPHERE, rec, x[:8, 42:45], x[:8, 45:48], x[:8, 48]).view(np.uint32), want[:8].view(np.uint32))


@pytest.mark.parametrize("shape", [0, 1, abi.MESH_INSTANCE, 0xfffffffb])
def test_hook_refuses_a_bad_shape(gpu, shape):
    x, out = np.zeros(64, F32), np.zeros(64, F32)
    assert gpu.lib().rspt_quadric_intersect(shape, x.ctypes.data, 1, out.ctypes.data) == abi.E_INVALID


# ---- rspt_trace ----
def mixed_scene(gpu, seed=13, mask="simple", n_each=120):
    """a few hundred triangles with overlapping spheres, disks and cylinders in declaration order: full and partial records, non-uniform and mirroring scales,
    shapes inside one another (a disk across a cylinder, a sphere inside it), and a disk coplanar with a triangle pair, so that a tie on t goes to whichever
    the leaf lists first.  mask: the second mesh's alpha / shadowalpha, as in tests/test_gpu_spheres.py (None | "simple" | "graph": ALPHA 0 | 2 | 1)."""
    rng = np.random.default_rng(seed)
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    zero = None if mask is None else sb.constant_texture(0.0)
    if mask == "graph":
        zero = sb.scale_texture(zero, sb.constant_texture(1.0))
    sb.add_quad([(-3, -3, 0), (3, -3, 0), (3, 3, 0), (-3, 3, 0)], mat)            # the plane z = 0 ...
    sb.add_disk(height=0.0, radius=2.5, innerradius=0.5, phimax=300.0, material=mat)   # ... and a disk in it (identity transform)
    for k in range(3):
        nt = 150
        c = rng.uniform(-8, 8, (nt, 1, 3))
        P = (c + rng.normal(size=(nt, 3, 3)) * 1.2).reshape(-1, 3)
        kw = dict(alpha=zero, shadow_alpha=zero) if (k == 1 and zero is not None) else {}
        sb.add_mesh(P.astype(F32), np.arange(3 * nt).reshape(-1, 3), mat, **kw)
        for _ in range(n_each // 3):
            scale = rng.uniform(0.6, 1.6, 3) * np.where(rng.uniform(size=3) < 0.1, -1, 1)
            m = xf(rng.uniform(-8, 8, 3), rng.normal(size=3), rng.uniform(0, 360), scale)
            r = float(rng.uniform(0.3, 2.0))
            partial = rng.integers(3)
            phimax = 360.0 if partial == 0 else float(rng.uniform(30, 330))
            sb.add_cylinder(radius=r, zmin=-float(rng.uniform(0.2, 2)), zmax=float(rng.uniform(0.2, 2)), phimax=phimax, object_to_world=m, material=mat)
            sb.add_disk(height=float(rng.uniform(-1, 1)), radius=1.3 * r, innerradius=0.0 if partial != 2 else 0.4 * r, phimax=phimax, object_to_world=m, material=mat)   # across it
            sb.add_sphere(0.6 * r, object_to_world=m, material=mat)                                                                                                     # inside it
            sb.add_disk(radius=float(rng.uniform(0.3, 2.0)), object_to_world=xf(rng.uniform(-8, 8, 3), rng.normal(size=3), rng.uniform(0, 360)), material=mat)
    return sb.finish(gpu.bvh_build)


def trace_instantiations(monkeypatch, capfd, run):
    monkeypatch.setenv("RSPT_VERBOSE", "1")
    capfd.readouterr()
    try:
        out = run()
    finally:
        err = capfd.readouterr().err
        monkeypatch.delenv("RSPT_VERBOSE")
        sys.stderr.write(err)
    return out, set(re.findall(r"rspt: trace instantiation '([^']+)'", err))


@pytest.mark.parametrize("mask,alpha", [(None, 0), ("simple", 2), ("graph", 1)])
def test_trace_mixed_scene_bit_exact(gpu, ref, monkeypatch, capfd, mask, alpha):
    sc = mixed_scene(gpu, mask=mask)
    mesh = sc.prims["mesh"]
    assert (mesh == abi.MESH_DISK).sum() >= 200 and (mesh == abi.MESH_CYLINDER).sum() >= 100 and (mesh == abi.MESH_SPHERE).sum() >= 100
    rng = np.random.default_rng(3)
    n = 1 << 14
    rays = np.zeros(n, abi.RAY_DT)
    rays["o"] = rng.uniform(-10, 10, (n, 3))
    d = rng.normal(size=(n, 3))
    rays["d"] = d / np.linalg.norm(d, axis=1)[:, None]
    # a quarter of the rays run straight down onto the coplanar disk / triangle pair: both report the same t there
    k = n // 4
    rays["o"][:k] = np.concatenate([rng.uniform(-2.9, 2.9, (k, 2)), np.full((k, 1), 0.75)], 1)
    rays["d"][:k] = (0, 0, -1)
    rays["t_max"] = np.where(rng.uniform(size=n) < 0.8, np.inf, rng.uniform(1, 15, n)).astype(F32)

    def walk(rr, any_hit):
        want = np.zeros(len(rr), abi.HIT_DT)
        ref.quad_walk(C.addressof(sc.desc), rr.ctypes.data, len(rr), any_hit, want.ctypes.data)
        return want

    with gpu.DeviceScene(sc) as ds:
        got, names = trace_instantiations(monkeypatch, capfd, lambda: gpu.trace(ds, rays))
        assert names == {"k_trace_w4quad<closest, alpha %d>" % alpha}       # a NEW instantiation served it, the one for this scene's masks
        want = walk(rays, 0)
        assert got.tobytes() == want.tobytes()
        hit = want["prim"] != abi.MISS
        by = mesh[want["prim"][hit]]
        for kind in (abi.MESH_DISK, abi.MESH_CYLINDER, abi.MESH_SPHERE):
            assert (by == kind).sum() > n // 100, kind
        assert (by < abi.MESH_CYLINDER).sum() > n // 100       # triangles
        # the coplanar pair: the straight-down rays that end on the plane z = 0 at the disk find the disk or the triangle by leaf order alone
        down = want[:k][(want["prim"][:k] != abi.MISS)]
        on_plane = down[np.abs(down["t"] - 0.75) < 1e-5]
        assert len(on_plane) > k // 8 and len(set(mesh[on_plane["prim"]])) == 2
        # secondary rays spawned just in front of the first hits, in random directions
        h = np.nonzero(hit)[0]
        sec = np.zeros(len(h), abi.RAY_DT)
        t = want["t"][h].astype(F32)
        sec["o"] = (rays["o"][h] + rays["d"][h] * (t * F32(0.9999))[:, None]).astype(F32)
        d2 = rng.normal(size=(len(h), 3))
        sec["d"] = d2 / np.linalg.norm(d2, axis=1)[:, None]
        sec["t_max"] = np.inf
        assert gpu.trace(ds, sec).tobytes() == walk(sec, 0).tobytes()
        for rr in (rays, sec):
            occ, names = trace_instantiations(monkeypatch, capfd, lambda: gpu.trace(ds, rr, any_hit=True))
            assert names == {"k_trace_w4quad<any, alpha %d>" % alpha}
            assert np.array_equal(occ["prim"], walk(rr, 1)["prim"])


def test_sphere_only_scene_keeps_the_sphere_kernels(gpu, ref, monkeypatch, capfd):
    """a scene with spheres and no disk or cylinder takes what it took: no quadric instantiation is named, and the hits equal the walk"""
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], mat)
    for c in ((0, 1, 0), (2, 0.5, 1), (-2, 1.5, -1)):
        sb.add_sphere(0.8, phimax=300.0, object_to_world=xf(c, (1, 1, 0), 30), material=mat)
    sc = sb.finish(gpu.bvh_build)
    rng = np.random.default_rng(1)
    rays = np.zeros(4096, abi.RAY_DT)
    rays["o"] = rng.uniform(-4, 4, (4096, 3)) + (0, 3, 0)
    d = rng.normal(size=(4096, 3))
    rays["d"] = d / np.linalg.norm(d, axis=1)[:, None]
    rays["t_max"] = np.inf
    with gpu.DeviceScene(sc) as ds:
        got, names = trace_instantiations(monkeypatch, capfd, lambda: gpu.trace(ds, rays))
    assert not names
    want = np.zeros(4096, abi.HIT_DT)
    ref.quad_walk(C.addressof(sc.desc), rays.ctypes.data, 4096, 0, want.ctypes.data)
    assert got.tobytes() == want.tobytes() and (sc.prims["mesh"][want["prim"][want["prim"] != abi.MISS]] == abi.MESH_SPHERE).sum() > 100


# ---- rspt_scene_create ----
def _room(gpu, shape, emit=None, point=False):
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], mat)
    if shape == "disk":
        sb.add_disk(radius=1.0, object_to_world=xf((0, 1, 0), (1, 0, 0), -90), material=mat, emit=emit)
    else:
        sb.add_cylinder(radius=0.5, zmin=0.0, zmax=1.0, object_to_world=xf((0, 0, 0), (1, 0, 0), -90), material=mat, emit=emit)
    if point:
        sb.add_point_light((0, 4, 0), (1.0, 1.0, 1.0))
    return sb.finish(gpu.bvh_build)


def _records(sc, shape):
    return sc.disks if shape == "disk" else sc.cylinders


def _refused(gpu, sc, code, word):
    with pytest.raises(gpu.RsptError) as e:
        gpu.DeviceScene(sc)
    assert e.value.code == code and word in str(e.value), str(e.value)


@pytest.mark.parametrize("shape", ["disk", "cylinder"])
def test_scene_create_validates_the_records(gpu, shape):
    good = _room(gpu, shape)
    with gpu.DeviceScene(good):
        pass
    mesh_code = abi.MESH_DISK if shape == "disk" else abi.MESH_CYLINDER

    def broken(field, value, index=None):
        sc = _room(gpu, shape)
        if index is None:
            _records(sc, shape)[field][0] = value
        else:
            _records(sc, shape)[field][0][index] = value
        return sc

    for sc in (broken("radius", 0.0), broken("radius", -1.0), broken("radius", np.nan), broken("radius", np.inf), broken("phi_max", 0.0), broken("phi_max", -0.5),
               broken("phi_max", 6.2832), broken("phi_max", np.nan), broken("object_to_world", np.inf, 3), broken("world_to_object", np.nan, 0),
               broken("medium_inside", 1)):
        _refused(gpu, sc, abi.E_INVALID, shape)
    if shape == "disk":
        for sc in (broken("inner_radius", 1.0), broken("height", np.nan), broken("inner_radius", np.inf)):
            _refused(gpu, sc, abi.E_INVALID, "disk")
    else:
        for sc in (broken("z_max", 0.0), broken("z_min", -np.inf), broken("z_max", np.nan)):
            _refused(gpu, sc, abi.E_INVALID, "cylinder")
    # the primitive's index
    sc = _room(gpu, shape)
    k = int(np.nonzero(sc.prims["mesh"] == mesh_code)[0][0])
    sc.prims["v"][k, 0] = 1
    _refused(gpu, sc, abi.E_INVALID, shape)
    sc = _room(gpu, shape)
    sc.prims["material"][k] = 7
    _refused(gpu, sc, abi.E_INVALID, shape)
    # a count without its array
    sc = _room(gpu, shape)
    setattr(sc.desc, "disks" if shape == "disk" else "cylinders", None)
    _refused(gpu, sc, abi.E_INVALID, shape)


@pytest.mark.parametrize("shape", ["disk", "cylinder"])
def test_scene_create_validates_the_light_pairing(gpu, shape):
    """area_light is -1 or a DIFFUSE_AREA light whose prim is that primitive, and such a light names it back; an emissive one is ACCEPTED here"""
    mesh_code = abi.MESH_DISK if shape == "disk" else abi.MESH_CYLINDER
    sc = _room(gpu, shape, emit=(1.0, 1.0, 1.0), point=True)
    k = int(np.nonzero(sc.prims["mesh"] == mesh_code)[0][0])
    assert sc.prims["area_light"][k] == 0 and sc.lights["prim"][0] == k and sc.lights["kind"][1] == abi.LIGHT_POINT
    with gpu.DeviceScene(sc):
        pass
    for bad in (-2, 1, 2):   # below -1; a point light; out of range
        sc.prims["area_light"][k] = bad
        _refused(gpu, sc, abi.E_INVALID, shape)
    sc.prims["area_light"][k] = -1   # the light names the primitive, the primitive names no light
    _refused(gpu, sc, abi.E_INVALID, shape)


@pytest.mark.parametrize("shape", ["disk", "cylinder"])
def test_with_instances_refused(gpu, shape):
    sc = _room(gpu, shape)
    inst = np.zeros(1, abi.INSTANCE_DT)
    obj = np.zeros(1, abi.OBJECT_DT)
    sc.desc.instances, sc.desc.n_instances = inst.ctypes.data, 1
    sc.desc.objects, sc.desc.n_objects = obj.ctypes.data, 1
    sc.desc.n_top_nodes, sc.desc.n_top_prims = len(sc.nodes), len(sc.prims)
    _refused(gpu, sc, abi.E_UNSUPPORTED, shape)
