#!/usr/bin/env python3
"""Lane occupancy of the shadow-ray kernel k_trace_w4q (csrc/trace_w4q.h) over the shadow rays of a short render: how many of a wave's 64 lanes its node
steps and its leaf phases run with, node steps and leaf visits per ray, and what an occluded ray walks, per leaf-phase threshold (RSPT_PW_LEAF_ANY_Q).
Needs the counter build of the library:
    AB_DEFS=-DRSPT_W4Q_COUNT tools/ab_build.sh count   ->   RSPT_LIB=exp/librspt_count.so python tools/w4q_lane_count.py
(timing-only: the counters cost registers and an occupancy step, so no rate of that build means anything).
usage: w4q_lane_count.py [--scenes soup1m,statue] [--spp 16] [--settings 8,16,32]
A setting is a threshold, or DEFER:threshold[:drain] for a library built with experiments/trace_w4q_deferred_leaves.patch (RSPT_ANY_Q_DEFER, RSPT_ANY_Q_DRAIN)."""
import argparse, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rs_pbrt_amd import scenes, lib

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", default="soup1m,statue")
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--settings", default="8,16,32")
args = ap.parse_args()
lib.init(0)
L = lib.lib()
if not hasattr(L, "rspt_w4q_count"):
    sys.exit("this librspt.so is not the counter build (AB_DEFS=-DRSPT_W4Q_COUNT)")
os.environ["RSPT_ANY_Q"] = "1"   # (every shadow-ray launch on the quantised records; no per-scene measurement)
out = (ctypes.c_ulonglong * 8)()
for name in args.scenes.split(","):
    if name == "soup1m":
        sc, rd = scenes.triangle_soup(lib.bvh_build, n_tris=1_000_000), scenes.soup_render_desc(res=1024, spp=args.spp, max_depth=8)
    else:
        sc, rd = scenes.statue_standin(lib.bvh_build), scenes.statue_render_desc(spp=args.spp)
    with lib.DeviceScene(sc) as ds:
        for setting in args.settings.split(","):
            f = setting.split(":") if ":" in setting else ["0", setting]
            os.environ["RSPT_ANY_Q_DEFER"], os.environ["RSPT_PW_LEAF_ANY_Q"], os.environ["RSPT_ANY_Q_DRAIN"] = f[0], f[1], (f[2] if len(f) > 2 else "0")
            L.rspt_w4q_count(out)   # (zero the counters)
            lib.render(ds, rd)
            if L.rspt_w4q_count(out) != 0:
                sys.exit("reading the counters failed")
            steps, step_lanes, phases, phase_lanes, occ, un, steps_occ, leaves_occ = [int(v) for v in out]
            rays = max(occ + un, 1)
            print(f"{name:7s} defer={f[0]} leaf={f[1]:>2s} drain={f[2] if len(f) > 2 else '0'}: rays {rays:10d} ({100.0 * occ / rays:4.1f} % occluded)  node steps {steps:10d} at {step_lanes / max(steps, 1):5.1f} lanes"
                  f"  leaf phases {phases:9d} at {phase_lanes / max(phases, 1):5.1f} lanes  wave-level steps + phases per ray {(steps + phases) / rays:7.4f}"
                  f"  per ray: steps {step_lanes / rays:6.2f} leaves {phase_lanes / rays:5.2f}; occluded: steps {steps_occ / max(occ, 1):6.2f} leaves {leaves_occ / max(occ, 1):5.2f}", flush=True)
