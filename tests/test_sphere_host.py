"""CPU: the host side of analytic spheres (ABI 23) — the rspt_sphere layout against the header, SceneBuilder.add_sphere's set-up values,
Sphere::world_bound, the mixed triangle / sphere aggregate, and the exporter's Shape "sphere" lines."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

from rs_pbrt_amd import abi, lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _libm():
    import ctypes.util
    L = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    L.acosf.restype = C.c_float
    L.acosf.argtypes = [C.c_float]
    return L


def test_sphere_layout_matches_the_header():
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "rspt.h"
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  printf("rspt_sphere %zu\n", sizeof(rspt_sphere)); printf("rspt_scene_desc %zu\n", sizeof(rspt_scene_desc));
  O(rspt_sphere, world_to_object); O(rspt_sphere, radius); O(rspt_sphere, phi_max); O(rspt_sphere, reverse_orientation);
  O(rspt_sphere, transform_swaps_handedness); O(rspt_sphere, medium_inside); O(rspt_sphere, medium_outside);
  O(rspt_scene_desc, media); O(rspt_scene_desc, spheres); O(rspt_scene_desc, n_spheres);
  printf("mesh_sphere %u\n", RSPT_MESH_SPHERE); printf("libm_sphere %d\n", (int)RSPT_LIBM_SPHERE); return 0; }'''
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "p.c"), "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "p"), os.path.join(td, "p.c")])
        out = dict(l.split() for l in subprocess.check_output([os.path.join(td, "p")]).decode().splitlines())
    assert int(out["rspt_sphere"]) == C.sizeof(abi.Sphere) == abi.SPHERE_DT.itemsize == 168
    assert int(out["rspt_scene_desc"]) == C.sizeof(abi.SceneDesc)
    for k, v in out.items():
        if "." in k:
            t, f = k.split(".")
            assert getattr({"rspt_sphere": abi.Sphere, "rspt_scene_desc": abi.SceneDesc}[t], f).offset == int(v), k
            if t == "rspt_sphere":
                assert abi.SPHERE_DT.fields[f][1] == int(v), k
    assert int(out["mesh_sphere"]) == abi.MESH_SPHERE and int(out["libm_sphere"]) == abi.LIBM_SPHERE
    # the scene description grew at its end only
    assert abi.SceneDesc.spheres.offset > abi.SceneDesc.media.offset


def test_add_sphere_setup_values():
    """Sphere::new (sphere.rs:59-84): z clamped to [-r, r] after min / max, theta from acosf of the UNCLAMPED z / r clamped to [-1, 1],
    phi_max = radians(clamp(phimax, 0, 360)) in f32; transform_swaps_handedness from the determinant's sign"""
    m = _libm()
    sb = scenes.SceneBuilder()
    sb.add_sphere(2.0, zmin=1.5, zmax=-3.0, phimax=400.0)
    mirror = scenes.Transform(np.diag([1.0, -1.0, 2.0, 1.0]).astype(F32))
    sb.add_sphere(0.5, zmin=-0.25, zmax=0.1, phimax=90.0, object_to_world=mirror)
    a, b = sb.spheres[0][0], sb.spheres[1][0]
    assert a["z_min"] == F32(-2.0) and a["z_max"] == F32(1.5)
    assert a["theta_min"] == F32(m.acosf(-1.0)) and a["theta_max"] == F32(m.acosf(F32(F32(1.5) / F32(2.0))))
    assert a["phi_max"] == F32(F32(F32(math.pi) / F32(180)) * F32(360))
    assert a["transform_swaps_handedness"] == 0 and b["transform_swaps_handedness"] == 1
    assert b["theta_min"] == F32(m.acosf(F32(F32(-0.25) / F32(0.5)))) and b["theta_max"] == F32(m.acosf(F32(F32(0.1) / F32(0.5))))
    assert b["phi_max"] == F32(F32(F32(math.pi) / F32(180)) * F32(90))
    assert np.array_equal(b["object_to_world"].reshape(4, 4), mirror.m) and np.array_equal(b["world_to_object"].reshape(4, 4), mirror.m_inv)
    assert a["reverse_orientation"] == 0


def test_sphere_world_bound():
    """Sphere::world_bound = object_to_world.transform_bounds(((-r, -r, z_min), (r, r, z_max))): the eight corners transformed in f32"""
    sb = scenes.SceneBuilder()
    xf = scenes.Transform.translate((10.0, -2.0, 3.0)) * scenes.Transform.scale(2.0, 1.0, 0.5)
    sb.add_sphere(1.5, zmin=-0.5, zmax=1.0, object_to_world=xf)
    lo, hi = scenes.sphere_world_bound(sb.spheres[0][0])
    assert np.array_equal(lo, np.array([10.0 - 3.0, -2.0 - 1.5, 3.0 - 0.25], F32))
    assert np.array_equal(hi, np.array([10.0 + 3.0, -2.0 + 1.5, 3.0 + 0.5], F32))


def _mixed(n_spheres=200, seed=1):
    rng = np.random.default_rng(seed)
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    P = rng.uniform(-10, 10, (300, 3)).astype(F32)
    sb.add_mesh(P, np.arange(300).reshape(-1, 3), mat)
    for i in range(n_spheres):
        sb.add_sphere(float(rng.uniform(0.1, 1.0)), object_to_world=scenes.Transform.translate(rng.uniform(-10, 10, 3)), material=mat,
                      emit=(1.0, 2.0, 3.0) if i % 50 == 0 else None)
    sb.add_mesh(P[:30] + F32(1), np.arange(30).reshape(-1, 3), mat)
    return sb


def test_mixed_aggregate_equals_the_oracle_builder():
    """the aggregate of a scene with spheres: rspt_bvh_build_bounds over the world bounds in declaration order, equal to the oracle's
    BVHAccel::new over the same bounds; prims carry the declaration-order primitive behind each slot"""
    from oracle import pyoracle
    sb = _mixed()
    sc = sb.finish(lib.bvh_build)
    bounds = []
    for kind, ref in sb.decl:
        if kind == "mesh":
            v = sb.P[ref][(sb.tris[ref] - sum(len(p) for p in sb.P[:ref])).astype(np.int64)]
            bounds += [np.concatenate([t.min(0), t.max(0)]) for t in v]
        else:
            lo, hi = scenes.sphere_world_bound(sb.spheres[ref][0])
            bounds.append(np.concatenate([lo, hi]))
    bounds = np.array(bounds, F32)
    nodes, ordered = pyoracle.bvh_build_bounds(bounds, 4)
    assert sc.nodes.tobytes() == nodes.tobytes()
    is_sph = sc.prims["mesh"] == abi.MESH_SPHERE
    assert is_sph.sum() == 200 and len(sc.prims) == 100 + 200 + 10
    decl_sph = np.array([k for kind, ref in sb.decl for k in ([ref] if kind == "sphere" else [-1] * len(sb.tris[ref]))])
    assert np.array_equal(sc.prims["v"][is_sph, 0], decl_sph[ordered[is_sph]])
    # one DiffuseAreaLight per emissive sphere, in declaration order
    assert len(sc.lights) == 4
    assert list(sc.prims["v"][sc.lights["prim"], 0]) == [0, 50, 100, 150]
    assert np.array_equal(sc.prims["area_light"][sc.lights["prim"]], np.arange(4))
    assert int(sc.desc.n_spheres) == 200


def test_exporter_writes_shape_sphere():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_pbrt
    sb = scenes.SceneBuilder()
    mat = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    sb.add_quad([(-5, 0, -5), (5, 0, -5), (5, 0, 5), (-5, 0, 5)], mat)
    xf = scenes.Transform(np.array([[2, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], F32))
    sb.add_sphere(0.75, zmin=-0.5, zmax=0.5, phimax=270.0, object_to_world=xf, material=mat, emit=(4.0, 4.0, 4.0))
    sc = sb.finish(lib.bvh_build)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "s.pbrt")
        export_pbrt.export(sc, path, ((0, 2, 8), (0, 1, 0), (0, 1, 0)), 45.0, 16, 16, 4)
        text = open(path).read()
    lines = [l.strip() for l in text.splitlines()]
    k = lines.index('Shape "sphere" "float radius" [0.75] "float zmin" [-0.5] "float zmax" [0.5] "float phimax" [270]')
    assert lines[k - 1] == "Transform [2 0 0 0 0 1 0 0 0 0 1 0 1 2 3 1]"
    assert lines[k - 3].startswith('AreaLightSource "diffuse" "rgb L" [4 4 4]')
    assert lines.index('Shape "trianglemesh"' + lines[[i for i, l in enumerate(lines) if l.startswith('Shape "trianglemesh"')][0]][len('Shape "trianglemesh"'):]) < k
