#!/usr/bin/env python3
"""Records fetched per packet by the masked packet walk (csrc/trace_packet.h) and by the frustum walk (csrc/trace_frustum.h) on the camera rays of the
C2 soup: how much larger the frustum walk's superset is; and per bundle by the bundle walk (csrc/trace_bundle.h) on 256 rays per pixel: whether a bundle of
R packets walks about the records of ONE packet, not R times that.  Needs the counter build of the library:
    AB_DEFS=-DRSPT_PK_COUNT tools/ab_build.sh count   ->   RSPT_LIB=exp/librspt_count.so python tools/pk_record_count.py
(timing-only: the counters cost an atomic per record, so no rate of that build means anything)."""
import argparse, ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rs_pbrt_amd import scenes, lib, abi

ap = argparse.ArgumentParser()
ap.add_argument("--tris", type=int, default=1_000_000)
ap.add_argument("--pixels", type=int, default=1 << 14)
ap.add_argument("--per", type=int, default=256, help="rays per pixel, in queue order (the headline: 256)")
args = ap.parse_args()
lib.init(0)
L = lib.lib()
if not hasattr(L, "rspt_pk_count_pk"):
    sys.exit("this librspt.so is not the counter build (AB_DEFS=-DRSPT_PK_COUNT)")
ds = lib.DeviceScene(scenes.triangle_soup(lib.bvh_build, n_tris=args.tris))
rng = np.random.default_rng(5)
side = int(np.sqrt(args.pixels)); yy, xx = np.mgrid[0:side, 0:side]
half = np.tan(np.radians(scenes.SOUP_FOV) / 2)
px = np.repeat(((xx.reshape(-1) + 0.5) / side - 0.5) * 2 * half, args.per) + rng.uniform(0, 2 * half / 1024, side * side * args.per)
py = np.repeat(((yy.reshape(-1) + 0.5) / side - 0.5) * 2 * half, args.per) + rng.uniform(0, 2 * half / 1024, side * side * args.per)
dd = np.stack([px, py, np.ones_like(px)], 1); dd /= np.linalg.norm(dd, axis=1)[:, None]
rays = np.zeros(len(px), abi.RAY_DT); rays["o"] = (0, 0, -4); rays["d"] = dd.astype(np.float32); rays["t_max"] = np.inf
out = (ctypes.c_ulonglong * 3)()
rows = {}
for label, value, fn in (("masked", "1", L.rspt_pk_count_pk), ("frustum", "2", L.rspt_pk_count_pf), ("bundle2", "3", L.rspt_pk_count_pb), ("bundle4", "4", L.rspt_pk_count_pb)):
    fn(out)   # (zero the counters)
    os.environ["RSPT_CAMERA_PACKET"] = value
    lib.trace(ds, rays)
    del os.environ["RSPT_CAMERA_PACKET"]
    if fn(out) != 0:
        sys.exit("reading the counters failed")
    rows[label] = (out[0], out[1], out[2])
    unit = "bundle" if label.startswith("bundle") else "packet"   # (a bundle kernel counts the bundles it walked as one; packets, where it handed a bundle to the packet code)
    print(f"{label:8s} {unit}s {out[2]:8d}  records/{unit} {out[0] / max(out[2], 1):7.1f}  leaf tests/{unit} {out[1] / max(out[2], 1):6.1f}  records per 256 rays {256.0 * out[0] / len(rays):7.1f}", flush=True)
print("records fetched: frustum / masked = %.3f" % (rows["frustum"][0] / max(rows["masked"][0], 1)))
