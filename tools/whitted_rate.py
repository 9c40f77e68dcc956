"""Rates of WhittedIntegrator and DirectLightingIntegrator ("all") on the same scenes, timed alternately in one process:
the C3 stand-in (statue, 1920x1080) and the Cornell box (512x512), 64 spp, depth 5, Sobol'.  rspt_render returns once the film is in
host memory, so the wall time around it is device-synchronised; warm-up renders of each pair come first.

    python tools/whitted_rate.py [--reps 3] [--scenes statue,cornell]

Prints one JSON line per (scene, integrator) with the best and median rate in Msamples/s."""
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
    ap.add_argument("--scenes", default="statue,cornell")
    args = ap.parse_args()
    from rs_pbrt_amd import lib, scenes
    lib.init(0)
    for name in args.scenes.split(","):
        if name == "statue":
            sc = scenes.statue_standin(lib.bvh_build_gpu)
            mk = lambda integ: scenes.statue_render_desc(xres=1920, yres=1080, spp=64, max_depth=5, integrator=integ,  # noqa: E731
                                                         light_samples=[1] * sc.desc.n_lights)
        elif name == "cornell":
            sc = scenes.cornell_box(lib.bvh_build_gpu)
            mk = lambda integ: scenes.cornell_render_desc(res=512, spp=64, max_depth=5, integrator=integ,  # noqa: E731
                                                          light_samples=[1] * sc.desc.n_lights)
        else:
            raise SystemExit("unknown scene %r" % name)
        descs = {integ: mk(integ) for integ in ("whitted", "directlighting")}
        times = {integ: [] for integ in descs}
        with lib.DeviceScene(sc) as ds:
            for _ in range(args.warmup):
                for rd in descs.values():
                    lib.render(ds, rd)
            for _ in range(args.reps):
                for integ, rd in descs.items():
                    t0 = time.perf_counter()
                    _, st = lib.render(ds, rd)
                    times[integ].append((time.perf_counter() - t0, st["samples"]))
        for integ, ts in times.items():
            rates = sorted(n / t / 1e6 for t, n in ts)
            print(json.dumps({"scene": name, "integrator": integ, "spp": 64, "max_depth": 5, "sampler": "sobol", "samples": ts[0][1],
                              "msamples_per_s_best": round(rates[-1], 1), "msamples_per_s_median": round(rates[len(rates) // 2], 1),
                              "seconds": [round(t, 4) for t, _ in ts]}), flush=True)
    lib.shutdown()


if __name__ == "__main__":
    main()
