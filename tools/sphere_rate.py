"""Rate of the path integrator on a frame of analytic spheres, and on the same frame with every sphere replaced by a tessellated triangle
sphere, timed alternately in one process: a ground quad and a grid of a few thousand spheres (matte, plastic, glass, metal, textured with a
bump map) under two triangle area lights and an infinite light, 1024x1024, 64 spp, depth 5, Sobol'.  rspt_render returns once the film is
in host memory, so the wall time around it is device-synchronised; warm-up renders of both scenes come first.

    python tools/sphere_rate.py [--reps 3] [--grid 56] [--res 1024] [--spp 64] [--tess 16]

Prints one JSON line per scene with the best and median rate in Msamples/s."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32 = np.float32


def uv_sphere(nv):
    """a unit sphere of 2 * nv * nv triangles with per-vertex normals and (u, v)"""
    nu = 2 * nv
    th = np.linspace(0.0, math.pi, nv + 1)
    ph = np.linspace(0.0, 2.0 * math.pi, nu + 1)
    t, p = np.meshgrid(th, ph, indexing="ij")
    P = np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], -1).reshape(-1, 3)
    UV = np.stack([p / (2 * math.pi), t / math.pi], -1).reshape(-1, 2)
    idx = []
    for i in range(nv):
        for j in range(nu):
            a, b, c, d = i * (nu + 1) + j, i * (nu + 1) + j + 1, (i + 1) * (nu + 1) + j, (i + 1) * (nu + 1) + j + 1
            if i > 0:
                idx.append((a, c, b))
            if i < nv - 1:
                idx.append((b, c, d))
    return P, UV, np.array(idx, np.int64)


def build(lib, scenes, grid, tess):
    """(sphere scene, tessellated scene): the same materials, lights and sphere transforms"""
    from tests.util import texture_image
    rng = np.random.default_rng(7)
    img = texture_image(64, 96)
    out = []
    for tessellated in (False, True):
        sb = scenes.SceneBuilder()
        height = sb.image_texture(img, channels=1, scale=0.03, trilinear=True)
        mats = [sb.add_material(scenes.matte((0.6, 0.55, 0.5))), sb.add_material(scenes.plastic((0.2, 0.3, 0.7), (0.4, 0.4, 0.4), 0.08)),
                sb.add_material(scenes.glass((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.5)), sb.add_material(scenes.metal(roughness=0.05)),
                sb.add_material(scenes.matte(sb.image_texture(img, su=2.0, sv=1.0), bump=height))]
        ground = sb.add_material(scenes.matte((0.4, 0.4, 0.4)))
        s = grid * 1.0
        sb.add_quad([(-s, 0, -s), (s, 0, -s), (s, 0, s), (-s, 0, s)], ground)
        sb.add_quad([(-6, 14, -6), (-2, 14, -6), (-2, 14, -2), (-6, 14, -2)], ground, emit=(30, 28, 25))
        sb.add_quad([(4, 12, 2), (8, 12, 2), (8, 12, 6), (4, 12, 6)], ground, emit=(20, 22, 28))
        sb.add_infinite_light((0.25, 0.3, 0.4))
        P0, UV0, I0 = uv_sphere(tess)
        r_all = rng.uniform(0.3, 0.45, grid * grid)
        m_all = rng.integers(len(mats), size=grid * grid)
        for k in range(grid * grid):
            i, j = divmod(k, grid)
            r = float(r_all[k])
            c = (-grid + 1.0 + 2.0 * j, r, -grid + 1.0 + 2.0 * i)
            m = np.eye(4, dtype=F32)
            m[:3, 3] = c
            if not tessellated:
                sb.add_sphere(r, object_to_world=scenes.Transform(m), material=mats[m_all[k]])
            else:
                sb.add_mesh((P0 * r + np.array(c)).astype(F32), I0, mats[m_all[k]], N=P0.astype(F32), UV=UV0.astype(F32))
        out.append(sb.finish(lib.bvh_build_gpu if tessellated else lib.bvh_build))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grid", type=int, default=56)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--tess", type=int, default=16, help="latitude bands of the triangle spheres (2 x tess x tess triangles each)")
    args = ap.parse_args()
    from rs_pbrt_amd import lib, scenes
    lib.init(0)
    sph, tri = build(lib, scenes, args.grid, args.tess)
    g = float(args.grid)
    rd = scenes.make_render_desc(args.res, args.res, args.spp, ((0.0, 0.35 * g, -1.15 * g), (0.0, 0.0, -0.1 * g), (0, 1, 0)), 45.0, max_depth=5, sampler="sobol")
    names = {"spheres": sph, "triangles": tri}
    times = {k: [] for k in names}
    ds = {k: lib.DeviceScene(v) for k, v in names.items()}
    try:
        for _ in range(args.warmup):
            for k in names:
                lib.render(ds[k], rd)
        for _ in range(args.reps):
            for k in names:
                t0 = time.perf_counter()
                _, st = lib.render(ds[k], rd)
                times[k].append((time.perf_counter() - t0, st["samples"]))
    finally:
        for d in ds.values():
            d.close()
    for k, ts in times.items():
        rates = sorted(n / t / 1e6 for t, n in ts)
        print(json.dumps({"scene": k, "spheres": args.grid * args.grid, "triangles": int(names[k].desc.n_prims) - (args.grid * args.grid if k == "spheres" else 0),
                          "res": args.res, "spp": args.spp, "max_depth": 5, "sampler": "sobol", "samples": ts[0][1],
                          "msamples_per_s_best": round(rates[-1], 1), "msamples_per_s_median": round(rates[len(rates) // 2], 1),
                          "seconds": [round(t, 4) for t, _ in ts]}), flush=True)
    lib.shutdown()


if __name__ == "__main__":
    main()
