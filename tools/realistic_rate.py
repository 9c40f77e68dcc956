"""Rate of the path integrator on the Cornell box under the realistic camera (ABI 26: tests/golden/lenses/dgauss50.dat, 35 mm film, 8 mm stop, focused on
the far wall) beside the perspective camera, timed alternately in one process on one upload of the scene: 256 x 256, 16 spp, depth 5, Sobol'.  The box
measures 555 units and the camera stands 800 in front of it, so the 50 mm lens sees about what the perspective camera's 39 degrees see.  rspt_render
returns once the film is in host memory, so the wall time around it is device-synchronised; warm-up renders under both cameras come first.

    python tools/realistic_rate.py [--reps 5] [--res 256] [--spp 16]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/realistic_rate.py --only realistic --reps 1 --warmup 0     (k_raygen_lens' share of one render)

Prints one JSON line per camera with the best and median rate in Msamples/s and the share of pixels that stayed black."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--only", choices=["perspective", "realistic"], default=None)
    args = ap.parse_args()
    import numpy as np
    from rs_pbrt_amd import lib, scenes
    lib.init(0)
    sc = scenes.cornell_box(lib.bvh_build)
    rds = {"perspective": scenes.cornell_render_desc(res=args.res, spp=args.spp, max_depth=5),
           "realistic": scenes.cornell_render_desc(res=args.res, spp=args.spp, max_depth=5, camera="realistic", film_diagonal=35.0, aperture_diameter=8.0,
                                                   focus_distance=1350.0, lens=os.path.join(ROOT, "tests", "golden", "lenses", "dgauss50.dat"))}
    if args.only:
        rds = {args.only: rds[args.only]}
    times = {k: [] for k in rds}
    dead = {}
    with lib.DeviceScene(sc) as ds:
        for _ in range(args.warmup):
            for k, rd in rds.items():
                lib.render(ds, rd)
        for _ in range(args.reps):
            for k, rd in rds.items():
                t0 = time.perf_counter()
                film, st = lib.render(ds, rd)
                times[k].append((time.perf_counter() - t0, st["samples"]))
                dead[k] = float((np.asarray(film)[:, :3].max(axis=1) == 0).mean())
    for k, ts in times.items():
        rates = sorted(n / t / 1e6 for t, n in ts)
        print(json.dumps({"camera": k, "res": args.res, "spp": args.spp, "max_depth": 5, "sampler": "sobol", "samples": ts[0][1], "black_pixels": round(dead[k], 4),
                          "msamples_per_s_best": round(rates[-1], 2), "msamples_per_s_median": round(rates[len(rates) // 2], 2),
                          "seconds": [round(t, 5) for t, _ in ts]}), flush=True)
    lib.shutdown()


if __name__ == "__main__":
    main()
