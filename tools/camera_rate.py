"""Rate of the path integrator on the C3 stand-in (scenes.statue_standin) under the three cameras rspt_render serves (ABI 25: perspective, orthographic,
environment), timed alternately in one process, each on its own upload of the scene: 1024x1024, 64 spp, depth 5, Sobol'.  The orthographic camera's screen window
frames the statue as the perspective camera does at its distance; the environment camera sits where the perspective camera sits and sees the whole
sphere of directions, most of which leave the scene.  rspt_render returns once the film is in host memory, so the wall time around it is
device-synchronised; warm-up renders under every camera come first.  They also carry tune_camera's one-off measurement, which is made once per scene
handle — hence one handle per camera: RSPT_VERBOSE=1 prints which camera-ray kernel each kept.

    python tools/camera_rate.py [--reps 3] [--grid 1466] [--res 1024] [--spp 64]

Prints one JSON line per camera with the best and median rate in Msamples/s."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    sc = scenes.statue_standin(lib.bvh_build_gpu, grid=args.grid)
    # fov 40 at distance ~4.24: half-width tan(20 deg) * 4.24 = 1.54 at the statue's centre
    rds = {cam: scenes.make_render_desc(args.res, args.res, args.spp, scenes.STATUE_LOOK_AT, 40.0, max_depth=5, sampler="sobol", camera=cam,
                                        screen_window=(-1.54, 1.54, -1.54, 1.54) if cam == "orthographic" else None)
           for cam in ("perspective", "orthographic", "environment")}
    times = {k: [] for k in rds}
    ds = {k: lib.DeviceScene(sc) for k in rds}
    try:
        for _ in range(args.warmup):
            for k, rd in rds.items():
                print("warm-up under the %s camera" % k, file=sys.stderr, flush=True)
                lib.render(ds[k], rd)
        for _ in range(args.reps):
            for k, rd in rds.items():
                t0 = time.perf_counter()
                _, st = lib.render(ds[k], rd)
                times[k].append((time.perf_counter() - t0, st["samples"], st["rays_closest"] + st["rays_any"]))
    finally:
        for d in ds.values():
            d.close()
    for k, ts in times.items():
        rates = sorted(n / t / 1e6 for t, n, _ in ts)
        print(json.dumps({"camera": k, "triangles": int(sc.desc.n_prims), "res": args.res, "spp": args.spp, "max_depth": 5, "sampler": "sobol", "samples": ts[0][1],
                          "rays": ts[0][2], "msamples_per_s_best": round(rates[-1], 1), "msamples_per_s_median": round(rates[len(rates) // 2], 1),
                          "seconds": [round(t, 4) for t, _, _ in ts]}), flush=True)
    lib.shutdown()


if __name__ == "__main__":
    main()
