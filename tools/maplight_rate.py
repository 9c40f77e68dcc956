"""Rate of the path integrator on the C3 stand-in (scenes.statue_standin) and on the same scene with a projection light and a goniometric light
added (ABI 24), timed alternately in one process: 1024x1024, 64 spp, depth 5, Sobol'.  The first scene runs the plastic shade instantiation and
the MOVE schedule; the second takes the generic-maplight instantiation with its slots kept for life, and a MIP lookup per delta-light sample.
rspt_render returns once the film is in host memory, so the wall time around it is device-synchronised; warm-up renders of both scenes come first.

    python tools/maplight_rate.py [--reps 3] [--grid 1466] [--res 1024] [--spp 64]

Prints one JSON line per scene with the best and median rate in Msamples/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32 = np.float32


def build(lib, scenes, grid):
    """(the stand-in, the stand-in + the two lights): the same arrays, the light list extended"""
    base = scenes.statue_standin(lib.bvh_build_gpu, grid=grid)
    rng = np.random.default_rng(24)
    sb = scenes.SceneBuilder()
    sb.add_projection_light((2.5, 2.8, -3.0), (0.0, 0.0, 0.0), (220, 210, 200), fov=30.0, image=rng.uniform(0.05, 1.0, (256, 512, 3)).astype(F32))
    sb.add_goniometric_light(scenes.Transform.translate((-2.0, 2.2, -1.5)), (40, 42, 44), image=rng.uniform(0.2, 1.0, (128, 256, 3)).astype(F32))
    lights = np.concatenate([base.lights, np.array(sb.delta_lights, base.lights.dtype)])
    lit = scenes.Scene(base.nodes, base.prims, base.meshes, base.P, base.N, base.UV, base.materials, lights, S=base.S, envmaps=sb.envmaps,
                       textures=base.textures, images=base.images, builder=base.builder)
    return base, lit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grid", type=int, default=1466)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    args = ap.parse_args()
    from rs_pbrt_amd import lib, scenes
    lib.init(0)
    base, lit = build(lib, scenes, args.grid)
    rd = scenes.make_render_desc(args.res, args.res, args.spp, scenes.STATUE_LOOK_AT, 40.0, max_depth=5, sampler="sobol")
    names = {"standin": base, "standin+maplights": lit}
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
        print(json.dumps({"scene": k, "triangles": int(names[k].desc.n_prims), "lights": int(names[k].desc.n_lights), "res": args.res, "spp": args.spp, "max_depth": 5,
                          "sampler": "sobol", "samples": ts[0][1], "msamples_per_s_best": round(rates[-1], 1), "msamples_per_s_median": round(rates[len(rates) // 2], 1),
                          "seconds": [round(t, 4) for t, _ in ts]}), flush=True)
    lib.shutdown()


if __name__ == "__main__":
    main()
