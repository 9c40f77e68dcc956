#!/usr/bin/env python3
"""Headline benchmark: Mpath-samples/s of the gfx950 wavefront path integrator on BASELINE.json
configs[1] — synthetic 1 M random-triangle soup, PathIntegrator depth 8, Sobol' 256 spp,
1024x1024 (resolution fixed by SURVEY.md §8d).

A "step" is one full render of that frame (1024*1024*256 = 268 M camera samples through
raygen -> trace -> shade -> film), with the scene already resident in HBM and the film left in HBM.
With N ranks the Morton-ordered 16x16 tiles of the frame are dealt to the ranks (strong scaling: the
frame is fixed) and the per-rank films are summed onto rank 0 by one ncclReduce INSIDE librspt
(rspt_render_desc.film_reduce, RCCL over xGMI) in the timed region.  Prints ONE JSON line on rank 0.

    python bench.py                       # N=1, 1 warm-up + 2 timed steps
    python bench.py --gpus 8              # spawns 8 ranks itself (torch.distributed.run) when WORLD_SIZE is unset
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 ... bench.py --gpus 8
    python bench.py --full                # the headline and everything below

A plain run does only what the headline needs: scene build and upload, the warm-up, the timed steps, --dump-outputs, the line.
Its `roofline` is a stub that says it was not measured.  With --full the line also carries (roofline at every N; the rest at N = 1,
rank 0 only; all of it outside the timed region of the headline):
  roofline       the traversal kernel (k_trace_w4, closest-hit + shadow-ray launches): its measured limiter (L1 request rate, from the
                 hash-matched PMC profile), its fabric-side traffic / the wall time of its launches against the 8 TB/s HBM peak, and
                 SURVEY 8(d)'s algorithmic bytes as a rate (not a fraction); the same for the shade stage under roofline.shade
  cpu_baseline   the C++ oracle's tile loop on all host cores on a bounded sample of the same frame (+ its 1-thread / all-thread scaling on one window)
  extra          C3 (the 4.3 M-triangle statue stand-in at 1920x1080x1024 spp — the north-star configuration) timed the
                 same way with its own roofline / cpu_baseline, and a 1/8-frame probe of the headline workload
                 (what one rank of an 8-GPU node renders)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s is what a streaming copy reaches)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sampler", default="sobol", choices=["sobol", "halton", "random", "02sequence", "stratified", "maxmindist"],
                    help="the four PCG-backed pixel samplers run one lane per 16x16 tile (a tile is one serial chain): a latency-bound workload")
    ap.add_argument("--integrator", default="path", choices=["path", "ao", "directlighting", "volpath"],
                    help="ao: AOIntegrator (64 cosine-sampled shadow rays per camera sample); directlighting: DirectLightingIntegrator, strategy all, maxdepth 5; "
                         "volpath: VolPathIntegrator (with --workload cornell the room is filled with a homogeneous medium)")
    ap.add_argument("--workload", default="soup1m", choices=["soup1m", "cornell", "cornell_docs", "statue", "statue_tex", "c4", "c5"])
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--lights", type=int, default=64, help="c4: number of small area lights (a square number; 64 = the C4 stand-in)")
    ap.add_argument("--filter", default="box", choices=["box", "gaussian"], help="pixel filter: the reference's default box 0.5 x 0.5, or gaussian radius 2 alpha 2 (every sample lands in ~16 pixels: k_film's splat path)")
    ap.add_argument("--alpha-mask", action="store_true", help="soup1m: every triangle carries an image alpha mask (the foliage case: k_trace_w4<.., ALPHA>)")
    ap.add_argument("--res", type=int, default=0)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--instancing", default="reference", choices=["reference", "fixed"], help="c5: what a hit inside an object instance is (rspt_scene_desc.instancing_mode)")
    ap.add_argument("--moving", action="store_true", help="c5: every instance is a MOVING TransformedPrimitive (two keys that differ by a rotation; k_trace_w4<INST, ANIM>)")
    ap.add_argument("--full", action="store_true", help="also the roofline (a counting pass of its own), the CPU baseline and, on the default configuration, "
                                                        "the C3 line and the 1/8-frame probe; the --no-* switches below drop parts of it")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the C3 line and the 1/8-frame probe")
    ap.add_argument("--no-count", action="store_true", help="skip the reference-order counting pass (no roofline block): for PMC runs")
    ap.add_argument("--cpu-spp", type=int, default=16, help="with --full: spp of the CPU baseline's sample of the frame")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="rank 0 writes what the last timed step computed to DIR/film.npy: the frame, float32 [pixels, 4] (xyz + filter weight), after the reduce; "
                         "a frame over 64 MB is cut to a fixed seeded sample of its pixels, whose indices go to DIR/film_pixels.npy (float64)")
    ap.add_argument("--watchdog", type=int, default=1500, help="seconds after which a rank that is still running dumps its stack and exits 1 (a hung collective "
                                                               "then ends the job with a non-zero code instead of holding the box); 0 = off")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def self_spawn(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU; on a box with fewer devices than
    ranks the ranks share devices and fall back to gloo — main()).  The launcher runs in its own process group under a time limit: a
    hung rank ends the run with a non-zero code."""
    import signal
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.Popen(cmd, env=env, start_new_session=True)
    try:
        return p.wait(timeout=(args.watchdog + 120) if args.watchdog > 0 else None)
    except subprocess.TimeoutExpired:
        sys.stderr.write("bench.py: the %d-rank job did not finish within %d s; killing its process group\n" % (args.gpus, args.watchdog + 120))
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        p.wait()
        return 124


PUBLISHED_CORNELL_MSAMPLES = 500 * 500 * 8 / (1024 / 1828.38) / 1e6   # 3.57


def ganesha_ply():
    """the largest .ply under $RSPT_GANESHA_DIR (the pbrt-v3 scenes' ganesha/geometry/ganesha.ply), or None"""
    d = os.environ.get("RSPT_GANESHA_DIR")
    if not d or not os.path.isdir(d):
        return None
    found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.lower().endswith(".ply")]
    return max(found, key=os.path.getsize) if found else None


def build_workload(args, workload, lib, scenes):
    """-> (scene, mk_rd(spp, shard), spp, name)"""
    integ = args.integrator
    if workload == "soup1m":
        res, spp = args.res or 1024, args.spp or 256
        sc = scenes.triangle_soup(lib.bvh_build_gpu, n_tris=args.tris, alpha_mask=args.alpha_mask)
        mk = lambda s, sh, **kw: scenes.soup_render_desc(res=res, spp=s, max_depth=8, shard=sh, integrator=integ, **kw)  # noqa: E731
        name = "synthetic %d-triangle soup%s, path depth 8, sobol %d spp, %dx%d" % (args.tris, ", every triangle under an image alpha mask" if args.alpha_mask else "", spp, res, res)
    elif workload == "cornell":
        res, spp = args.res or 400, args.spp or 64
        sc = scenes.cornell_box(lib.bvh_build_gpu, fog=scenes.CORNELL_FOG if integ == "volpath" else None)
        mk = lambda s, sh, **kw: scenes.cornell_render_desc(res=res, spp=s, shard=sh, integrator=integ, **kw)  # noqa: E731
        name = "Cornell Box%s, path depth 5, sobol %d spp, %dx%d" % (" filled with a homogeneous medium (optical depth ~1 across the room)" if integ == "volpath" else "", spp, res, res)
    elif workload == "cornell_docs":
        # the ONE configuration the reference publishes a rate for (docs/source/getting_started.rst:161-175, 500 x 500, sobol 8 spp, path,
        # 1828.38 tiles/s on 28 threads = 3.57 Msamples/s), on the scene recovered from the reference's own renders of it
        res, spp = args.res or 500, args.spp or 8
        sc = scenes.cornell_box_docs(lib.bvh_build_gpu)
        mk = lambda s, sh, **kw: scenes.cornell_docs_render_desc(s, res, shard=sh, integrator=integ, **kw)  # noqa: E731
        name = "the Cornell box of the reference's documentation (scene recovered from its renders, 94 %% of the 8-spp PNG reproduced byte for byte), path depth 5, sobol %d spp, %dx%d" % (spp, res, res)
    elif workload == "c5":
        xres, spp = args.res or 1920, args.spp or 64
        yres = xres * 9 // 16
        sc = scenes.landscape_standin(lib.bvh_build_gpu, instancing=args.instancing, moving=args.moving)
        mk = lambda s, sh, **kw: scenes.landscape_render_desc(xres=xres, yres=yres, spp=s, shard=sh, integrator=integ, **kw)  # noqa: E731
        name = "landscape stand-in (4096 instances of a 10 k-triangle tree + lat-long sky; DECLARED STAND-IN for the off-tree Landscape scene; instancing mode %s%s), path depth 5, sobol %d spp, %dx%d" % (args.instancing, "; every instance moving over the shutter" if args.moving else "", spp, xres, yres)
    else:
        xres, spp = args.res or 1920, args.spp or 1024
        yres = xres * 9 // 16
        tex = workload in ("statue_tex", "c4")  # image-textured Kd + bump map + textured ground
        mk = lambda s, sh, **kw: scenes.statue_render_desc(xres=xres, yres=yres, spp=s, shard=sh, integrator=integ, **kw)  # noqa: E731
        ply = ganesha_ply() if workload == "statue" else None
        if ply:   # SURVEY 8(d) / BASELINE.md: the real 4.3 M-triangle mesh when the off-tree asset is supplied
            sc, n_tri = scenes.statue_from_ply(lib.bvh_build_gpu, ply)
            name = "Ganesha mesh %s (%d triangles, from $RSPT_GANESHA_DIR) in the stand-in's frame: its camera, ground, three quad lights, plastic; path depth 5, sobol %d spp, %dx%d" % (
                os.path.basename(ply), n_tri, spp, xres, yres)
        else:
            sc = scenes.statue_standin(lib.bvh_build_gpu, textured=tex, many_lights=args.lights if workload == "c4" else 0)  # c4: SURVEY 8(d) C4 stand-in
            name = "statue stand-in (4.3 M triangles%s%s; DECLARED STAND-IN for the off-tree Ganesha asset), path depth 5, sobol %d spp, %dx%d" % (
                ", image-textured + bump-mapped" if tex else "", ", %d small area lights (C4 stand-in)" % args.lights if workload == "c4" else "", spp, xres, yres)
    if integ != "path":
        name += " [%s integrator]" % integ
    if args.filter == "gaussian":
        plain_mk = mk

        def mk(s, sh, **kw):  # noqa: E731
            return plain_mk(s, sh, filter_radius=(2.0, 2.0), filter_table=scenes.gaussian_filter_table((2.0, 2.0), 2.0), **kw)
        name += " [gaussian filter, radius 2]"
    if args.sampler != "sobol":   # the default of every workload above
        base_mk = mk

        def mk(s, sh, **kw):  # noqa: E731
            extra = {}
            if args.sampler == "stratified":   # xsamples x ysamples = the (power-of-two) sample count
                k = max(int(s).bit_length() - 1, 0)
                extra["strat"] = (1 << ((k + 1) // 2), 1 << (k // 2))
            return base_mk(s, sh, sampler=args.sampler, **extra, **kw)
        name = name.replace("sobol", args.sampler)
        if args.sampler not in ("sobol", "halton"):
            name += " [pixel sampler: one lane per 16x16 tile, a tile is one serial chain of its PCG32 stream]"
    return sc, mk, spp, name


def measured_traffic(lib, workload, default_cfg):
    """PMC figures of one step from the committed rocprofv3 passes (profiles/rNN_pmc_traffic.json, written by tools/refresh_profiles.sh +
    tools/pmc_to_json.py: FETCH_SIZE / WRITE_SIZE in separate passes with the gfx950 correction of MI355X_MICROARCH.md; TCP / SQ / TA passes
    for the limiter ratios).  PMC counters cannot be read from inside this process, so the figures are only quoted as current when the
    profile was taken with the same kernel sources (hash of rs_pbrt_amd/csrc + include/rspt.h) and for the exact workload; a profile of
    other sources is passed on marked stale and never enters a ratio.  -> (record | None, note | None, stale record | None)"""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")))
    if not files:
        return None, "no profiles/rNN_pmc_traffic.json", None
    stale = None
    for f in reversed(files):
        try:
            t = json.load(open(f))
        except (OSError, ValueError):
            continue
        w = t.get("workloads", {}).get(workload)
        if not default_cfg or not w:
            continue
        w = dict(w, file=os.path.relpath(f, ROOT), source_hash=t.get("source_hash"))
        if t.get("source_hash") == lib.source_hash():
            return w, None, None
        stale = stale or w
    if stale:
        return None, "newest PMC pass (%s) is from other kernel sources (%s, library %s)" % (stale["file"], stale["source_hash"], lib.source_hash()), stale
    return None, "no PMC pass for this workload / size", None


DEVICE = {"cus": 256, "clock_ghz": 2.4}   # MI355X; main() overwrites both from the running device


def roofline_block(counts, count_scale, stats, traffic, traffic_note, stale, ms_per_step):
    """The dominant kernel k_trace_w4 (closest-hit + shadow-ray launches of one step, this rank) and, under "shade", the second one.

    `bound` is the MEASURED limiter: the per-lane record loads saturate the CU's L1 request path
    (l1_request_frac = TCP line probes per CU per cycle, ceiling 1) with VALU issue close behind; HBM is not it.  The HBM figures
    (`achieved`, `frac`, `traffic`) are what the contract asks to see next to that: fabric-side bytes from the PMC passes (an upper bound of
    HBM bytes: Infinity-Cache hits included) / the WALL time of the trace launches (closest-hit and shadow-ray launches overlap on two streams;
    their summed durations would count that time twice).  SURVEY 8(d)'s algorithmic bytes (32 B per node visit + 48 B per triangle test of
    the REFERENCE's traversal + queue records) are reported as `alg_bytes_per_launch` / `alg_rate_gbs`, NOT as a fraction of the HBM peak:
    the four-box kernel fetches half as many, larger records and most of them from L2 / Infinity Cache, so that rate may exceed 8 TB/s."""
    n = len(stats)
    trace_bytes = count_scale * (32.0 * counts["nodes_visited"] + 48.0 * counts["tris_tested"] + 96.0 * counts["rays_closest"] + 72.0 * counts["rays_any"])
    t_c = sum(s["t_trace_closest_s"] for s in stats) / n
    t_a = sum(s["t_trace_any_s"] for s in stats) / n
    t_wall = sum(s["t_trace_s"] for s in stats) / n
    if t_wall <= 0.0:   # schedules that run their trace launches one after the other on one stream (volpath, directlighting): the sum is the wall time
        t_wall = t_c + t_a
    t_sh = sum(s["t_shade_s"] for s in stats) / n
    t_k = sum(s["t_kernels_s"] for s in stats) / n
    launches = stats[0]["launches_closest"] + stats[0]["launches_any"]
    rays = count_scale * (counts["rays_closest"] + counts["rays_any"])
    # every duration that enters a ratio below is a wall time inside the step
    assert t_wall <= ms_per_step * 1e-3 * 1.02 and t_sh <= ms_per_step * 1e-3 * 1.02 and t_wall + t_sh <= t_k * 1.02, (t_wall, t_sh, t_k, ms_per_step)
    lim = (traffic or {}).get("limiters", {})
    lc, la = lim.get("trace_closest", {}), lim.get("trace_any", {})
    miss_lines = (lc.get("l1_miss_lines") or 0.0) + (la.get("l1_miss_lines") or 0.0)
    out = {"bound": "l1", "bound_detail": "the CU's L1 request path: every lane of a node step reads its own 128-byte record with seven 16-byte loads, and a CU's L1 takes ONE such divergent lane "
                                          "request per clock (l1_request_frac = TCP_TOTAL_CACHE_ACCESSES / CU / clock, ceiling 1) — with VALU issue right behind (valu_busy).  Round 5's model sweeps "
                                          "(profiles/r05_w8_sweeps.txt) settle what the walk is NOT bound by: occupancy (1 workgroup per CU runs as fast as 8: not latency x misses in flight), the L2 hit "
                                          "rate short of 1 (0.63 -> 0.85 is +4 %), per-XCD locality (no faster than a shared hot set; XCD-affine dealing measured neutral, profiles/r05_xcd_affine_ab.txt), "
                                          "HBM (frac below), MFMA (none)",
           "binding_frac": lim.get("trace_closest", {}).get("l1_request_frac"),
           "kernel": "k_trace_w4 (BVH traversal + triangle test; closest-hit + shadow-ray launches)",
           "l1_request_frac": lim.get("trace_closest", {}).get("l1_request_frac"), "ta_busy": lim.get("trace_closest", {}).get("ta_busy"),
           "valu_busy": lim.get("trace_closest", {}).get("valu_busy"),
           # the L1-miss side (TCP_TCC_READ_REQ of the same PMC pass): lines per ray, their mean latency, how many a CU keeps in flight, and the line rate over
           # the launches' wall time; a random walk with this kernel's shape reaches ~60 G lines/s on this GPU (profiles/r04_step_model.txt)
           "l1_miss_lines_per_ray": (miss_lines / rays) if miss_lines else None,
           "l1_miss_latency_cycles": lc.get("l1_to_l2_read_latency_cycles"), "l1_misses_in_flight_per_cu": lc.get("l1_misses_in_flight_per_cu"),
           "l1_hit_rate": lc.get("l1_hit_rate"), "l2_hit_rate": lc.get("l2_hit_rate"),
           "l1_miss_g_lines_per_s": (miss_lines / t_wall / 1e9) if miss_lines else None,
           "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None,
           "launches_per_step": launches, "avg_launch_ms": t_wall / max(launches, 1) * 1e3,
           # per-launch HIP-event durations, the figures rocprofv3 --kernel-trace --stats reports as "avg" for the two instantiations (profiles/rNN_soup1m_kernel_stats.md)
           "avg_launch_ms_by_kernel": {"k_trace_w4<closest>": t_c / max(stats[0]["launches_closest"], 1) * 1e3, "k_trace_w4<any>": t_a / max(stats[0]["launches_any"], 1) * 1e3},
           "alg_bytes_per_launch": trace_bytes / max(launches, 1), "alg_rate_gbs": trace_bytes / t_wall / 1e9, "alg_bytes_per_step_rank0": trace_bytes,
           "how": "achieved = PMC fabric-side bytes of the step's trace launches (FETCH_SIZE x 2 + WRITE_SIZE, MI355X_MICROARCH.md) / their wall time (%.3f s; "
                  "per-launch HIP-event durations sum to %.3f s because the shadow-ray launch of a bounce overlaps the closest-hit launch on a second stream); "
                  "frac = achieved / 8 TB/s; l1_request_frac / ta_busy / valu_busy from the TCP / TA / SQ passes of the same profile" % (t_wall, t_c + t_a),
           "seconds_per_step": {"trace_closest_launches": t_c, "trace_any_launches": t_a, "trace_wall_overlapped": t_wall, "shade_launches": t_sh, "all_kernels_wall": t_k},
           "whole_path_alg_bytes_per_sample": counts["alg_bytes"] / max(counts["samples"], 1),
           "rays_per_sample": (counts["rays_closest"] + counts["rays_any"]) / max(counts["samples"], 1),
           "nodes_per_ray": counts["nodes_visited"] / max(counts["rays_closest"] + counts["rays_any"], 1),
           "tris_per_ray": counts["tris_tested"] / max(counts["rays_closest"] + counts["rays_any"], 1),
           "mrays_per_s": rays / t_wall / 1e6}
    # three more fractions, each against the ceiling it names:
    #   alg_frac       SURVEY 8(d)'s algorithmic bytes / SUM of the per-launch durations / 8 TB/s — the contract's literal "achieved / peak".  It can
    #                  exceed 1 and does: the model prices every node visit of the REFERENCE's traversal as a fresh 32-byte HBM fetch, the kernel
    #                  fetches half as many 128-byte records and nearly all of them from L2 / Infinity Cache — it is not a bound, it is printed as asked
    #   l2_line_frac   L1-miss lines x 128 B / wall time of the launches / 34.5 TB/s (aggregate L2 -> L1 bandwidth, MI355X_MICROARCH.md: 2048 B/clk/XCD)
    #   latency_bound_g_lines_per_s   misses in flight per CU x 256 CUs / mean miss latency: the rate Little's law allows at THIS latency and THIS
    #                  number of outstanding misses; l1_miss_g_lines_per_s sits on it by construction over the kernels' busy cycles — what can move is
    #                  the latency (the L2 hit rate) and the number in flight (occupancy), which is what profiles/r05_w8_sweeps.txt varies
    L2_PEAK_GBS, CLOCK_GHZ, N_CUS = 34500.0, DEVICE["clock_ghz"], DEVICE["cus"]   # (the device's own figures: main() fills DEVICE from torch's device properties)
    out["alg_frac"] = trace_bytes / (t_c + t_a) / 1e9 / HBM_PEAK_GBS if (t_c + t_a) > 0 else None
    out["alg_frac_note"] = "SURVEY 8(d) bytes / summed launch durations / 8 TB/s; > 1 means the byte model over-counts (L2 / Infinity-Cache residency, four-box records), not that HBM is saturated"
    out["l2_line_frac"] = (miss_lines * 128.0 / t_wall / 1e9 / L2_PEAK_GBS) if miss_lines else None
    lat, infl = lc.get("l1_to_l2_read_latency_cycles"), lc.get("l1_misses_in_flight_per_cu")
    out["latency_bound_g_lines_per_s"] = (infl * N_CUS / lat * CLOCK_GHZ) if (lat and infl) else None
    if out["l1_request_frac"] is None:   # no PMC pass of THIS source hash: the limiter was not measured for this build, say so instead of naming one
        out["bound"] = "l1 (as measured on the last profiled build; no PMC pass for this source hash, binding_frac null)"
    # the shade stage (k_bin_* + k_texture + k_shade): SURVEY 8(d) prices it at 48 B per closest-hit ray (32 B ray record written + 16 B hit record
    # read) + 36 B per shadow ray (32 B written + 4 B flag read) + 96 B of path state per bounce
    n_bounce = count_scale * (counts["alg_bytes"] - 32.0 * counts["samples"]) / 96.0 - trace_bytes / 96.0
    shade_alg = 48.0 * count_scale * counts["rays_closest"] + 36.0 * count_scale * counts["rays_any"] + 96.0 * n_bounce
    sh = {"bound": "hbm", "bound_detail": "bytes of path state moved per path and bounce (scattered 16 - 32-byte records of the SoA slot, ~3.2 x SURVEY 8(d)'s budget) at 2 - 3 waves / SIMD; "
                                          "issuing every slot load up front (fewer dependent round trips, 68 more bytes per path) lost 4 %: experiments/README.md round 4",
          "kernel": "k_shade (+ k_bin_*, k_texture)", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None,
          "alg_bytes_per_step": shade_alg, "alg_rate_gbs": shade_alg / t_sh / 1e9 if t_sh > 0 else None, "seconds_per_step": t_sh,
          "valu_busy": lim.get("shade", {}).get("valu_busy"), "wait_frac": lim.get("shade", {}).get("wait_frac"), "waves_per_simd": lim.get("shade", {}).get("waves_per_simd")}
    if traffic:
        tb = traffic["trace_traffic_bytes_per_step"]
        out["achieved"] = tb / t_wall / 1e9
        out["frac"] = out["achieved"] / HBM_PEAK_GBS
        out["traffic"] = tb / max(launches, 1)
        out["traffic_over_algorithmic"] = tb / trace_bytes
        out["traffic_source"] = "%s (source hash %s = this library)" % (traffic["file"], traffic["source_hash"])
        sb = traffic.get("shade_traffic_bytes_per_step")
        if sb and t_sh > 0:
            sh["achieved"] = sb / t_sh / 1e9
            sh["frac"] = sh["achieved"] / HBM_PEAK_GBS
            sh["traffic"] = sb
            sh["traffic_over_algorithmic"] = sb / shade_alg
        for fr in (out["frac"], sh["frac"], out["l1_request_frac"], out["ta_busy"], out["valu_busy"]):
            assert fr is None or 0.0 <= fr <= 1.0, "a printed fraction left [0, 1]: %r" % fr
    else:
        out["traffic_note"] = traffic_note
        if stale:   # shown, marked, in no ratio
            out["stale_profile"] = {"file": stale["file"], "source_hash": stale["source_hash"], "trace_traffic_bytes_per_step": stale["trace_traffic_bytes_per_step"],
                                    "limiters": stale.get("limiters")}
    out["shade"] = sh
    return out


DUMP_BYTES_MAX = 64 << 20


def dump_outputs(d, film):
    """the last timed step's frame as DIR/film.npy; over DUMP_BYTES_MAX, the same fixed seeded sample of pixels every run (indices in film_pixels.npy)"""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    rows_max = (DUMP_BYTES_MAX - 4096) // (film.itemsize * film.shape[1] + 8)   # (8: a float64 pixel index per sampled row; 4096: the two .npy headers)
    if film.nbytes > DUMP_BYTES_MAX - 4096:
        idx = np.sort(np.random.default_rng(20261015).choice(film.shape[0], rows_max, replace=False))
        film = film[idx]
        np.save(os.path.join(d, "film_pixels.npy"), idx.astype(np.float64))
    elif os.path.exists(os.path.join(d, "film_pixels.npy")):
        os.remove(os.path.join(d, "film_pixels.npy"))   # (left by an earlier, larger frame: film.npy is whole now)
    np.save(os.path.join(d, "film.npy"), np.ascontiguousarray(film, np.float32))


def time_steps(step, fence, n):
    fence()
    t0 = time.perf_counter()
    stats = [step() for _ in range(n)]
    fence()
    return time.perf_counter() - t0, stats


def host_cpu_facts():
    """what the box gives this process: logical CPUs, the affinity mask, the cgroup CPU quota (a container may see 256 CPUs and be allowed 32)"""
    facts = {"logical_cpus": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None, "cgroup_cpu_max": None, "model": None}
    for f in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            facts["cgroup_cpu_max"] = open(f).read().strip()
            break
        except OSError:
            pass
    try:
        facts["model"] = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    return facts


def effective_cores():
    """the cores this process may actually use: the affinity mask, cut by the cgroup CPU quota (the GPU boxes show 256 logical CPUs to a container that is
    allowed 16 CPUs' worth of time — 256 threads then run at 16 cores' speed, which is what rounds 1-4 reported as "256 cores")"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, -(-q // per)))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(args, pyoracle, sc, mk_rd, spp, scaling_crop):
    ncores = effective_cores()
    rd_cpu = mk_rd(spp, (0, 1, 64))
    def cpu_render(rd_, threads):
        if args.integrator != "directlighting":
            return pyoracle.render(sc, rd_, threads=threads)
        t0 = time.perf_counter()  # the oracle's recursive_li (directlighting.rs), strategy all, one sample per light
        r_ = pyoracle.render_integrator(sc, rd_, "direct", threads=threads)
        r_["seconds"] = time.perf_counter() - t0
        return r_

    r = cpu_render(rd_cpu, ncores)
    c = r["counters"]
    out = {"value": c["samples"] / r["seconds"] / 1e6, "unit": "Msamples/s", "cores": ncores, "kind": "port",
           "sample": "same scene and frame at %d spp (%d samples), C++ oracle restatement of rs_pbrt's tile loop (rs_pbrt itself cannot be built "
                     "here: no Rust toolchain), %d threads = the cores this container may use (affinity cut by the cgroup CPU quota; cpu_baseline.host), %.1f s" % (spp, c["samples"], ncores, r["seconds"]),
           # SURVEY 8(d) "oracle_counters.json per config", emitted in the run: the CPU oracle's own node / triangle / ray counts
           "oracle_counters_per_sample": {"nodes": c["nodes_visited"] / c["samples"], "tris": c["tris_tested"] / c["samples"],
                                          "rays_closest": c["rays_closest"] / c["samples"], "rays_any": c["rays_any"] / c["samples"],
                                          "alg_bytes": (32.0 * c["nodes_visited"] + 48.0 * c["tris_tested"] + 96.0 * c["rays_closest"] + 72.0 * c["rays_any"]
                                                        + 96.0 * c["bounces"] + 32.0 * c["samples"]) / c["samples"]}}
    # how the port scales with threads, on ONE sample for both runs: a crop window of 256 tiles (one per hardware thread of the box) at an spp chosen so
    # that the all-thread leg runs for >= 2 s at the rate just measured (legs of 0.0 - 0.4 s measured thread start-up, not rendering);
    # the one-thread leg is then that many seconds x the ratio
    crop_px = 256 * 256
    spp_s = 1
    while crop_px * spp_s < 2.2e6 * out["value"] and spp_s < 4096:
        spp_s *= 2
    rp = cpu_render(mk_rd(1, (0, 1, 64), crop=scaling_crop), 1)                      # probe: bounds the one-thread leg to ~40 s
    v1_probe = rp["counters"]["samples"] / max(rp["seconds"], 1e-6)
    while spp_s > 1 and crop_px * spp_s > 40.0 * v1_probe:
        spp_s //= 2
    rd_s = mk_rd(spp_s, (0, 1, 64), crop=scaling_crop)
    rn, r1 = cpu_render(rd_s, ncores), cpu_render(rd_s, 1)
    v1, vn = r1["counters"]["samples"] / r1["seconds"] / 1e6, rn["counters"]["samples"] / rn["seconds"] / 1e6
    out["thread_scaling"] = {"ratio": vn / v1, "one_thread": v1, "all_threads": vn, "unit": "Msamples/s",
                             "sample": "crop window %s of the frame at %d spp (%d samples) for BOTH runs: 1 thread %.1f s, %d threads %.1f s (the tile loop hands out 16x16 tiles: "
                                       "%d tiles in this window)" % (list(rd_s.crop_px), spp_s, r1["counters"]["samples"], r1["seconds"], ncores, rn["seconds"],
                                                                     ((rd_s.crop_px[2] - rd_s.crop_px[0] + 15) // 16) * ((rd_s.crop_px[3] - rd_s.crop_px[1] + 15) // 16))}
    out["host"] = host_cpu_facts()
    return out


def measure(args, lib, scenes, workload, steps, warmup, shard, world, reduce_in_lib, torch_reduce, fence, count_spp_div=1, rank0=True):
    """scene build + upload + counting pass + warm-up + timed steps for one workload on this rank"""
    import torch
    t0 = time.time()
    sc, mk_rd, spp, wl_name = build_workload(args, workload, lib, scenes)
    rd = mk_rd(spp, shard)
    rd.film_reduce = 1 if reduce_in_lib else 0
    t_scene = time.time() - t0
    t0 = time.time()
    ds = lib.DeviceScene(sc)
    t_upload = time.time() - t0
    film = torch.zeros(scenes.n_pixels(rd) * 4, dtype=torch.float32, device="cuda")
    film_host = torch.zeros(scenes.n_pixels(rd) * 4, dtype=torch.float32).pin_memory() if rank0 else None

    def step():
        st = lib.render_device(ds, rd, film.data_ptr())  # the reduce (N > 1) runs inside, on the library's stream, before it returns
        if torch_reduce:
            torch_reduce(film)
        if film_host is not None:   # t_render ends with the film in host memory (rank 0 holds the frame)
            film_host.copy_(film)
        return st

    # counting pass (deterministic: identical counts in the timed passes) for the algorithmic-bytes roofline; rank-local, no reduce.  A plain run
    # without warm-up makes it too: it is the render that allocates the path buffers and loads the kernels ahead of the first timed step
    counts = None
    if not args.no_count and (args.full or warmup == 0) and args.sampler in ("sobol", "halton"):   # (the tile-serial kernel of the pixel samplers has no counting variant)
        rd_count = mk_rd(max(spp // count_spp_div, 1), shard)
        os.environ["RSPT_COUNTERS"] = "1"
        counts = lib.render_device(ds, rd_count, film.data_ptr())
        os.environ["RSPT_COUNTERS"] = "0"
    for _ in range(warmup):
        step()
    elapsed, stats = time_steps(step, fence, steps)
    return dict(sc=sc, ds=ds, mk_rd=mk_rd, spp=spp, name=wl_name, rd=rd, counts=counts, count_scale=float(spp) / max(spp // count_spp_div, 1),
                elapsed=elapsed, stats=stats, t_scene=t_scene, t_upload=t_upload, film=film, step=step, film_host=film_host)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_spawn(args))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.watchdog > 0:   # a rank that is still here after this long is hung (a collective one member never entered): stack to stderr, exit 1 —
        import faulthandler  # torch.distributed.run then stops the other ranks and the job ends with a non-zero code
        faulthandler.dump_traceback_later(args.watchdog, exit=True)
    import torch  # first, so librspt binds to the HIP runtime torch already loaded
    import torch.distributed as dist
    from rs_pbrt_amd import lib, multigpu, scenes
    n_dev = max(torch.cuda.device_count(), 1)
    # fewer devices than ranks (a one-GPU box running the N > 1 control flow): ranks share devices, and the transport is gloo over host
    # memory — RCCL refuses two ranks on one device ("Duplicate GPU detected").  Same spawn, uid exchange, tile deal, film sum, max-over-ranks
    # time and JSON line as on a full node; the rate it prints is that of one oversubscribed GPU and says so.
    shared_devices = world > n_dev
    device_index = local_rank % n_dev
    torch.cuda.set_device(device_index)
    # ONE librccl per process and one policy everywhere (rspt_comm_library, include/rspt.h): the copy the process has mapped already — torch's,
    # since torch is imported first here and in the tests — else $RSPT_RCCL_LIB, else the loader's.  The path that was bound is printed in the line.
    lib.init(device_index)
    try:
        props = torch.cuda.get_device_properties(device_index)
        DEVICE["cus"] = int(props.multi_processor_count) or 256
        DEVICE["clock_ghz"] = (float(getattr(props, "clock_rate", 0)) / 1e6) or 2.4
    except Exception:  # noqa: BLE001
        pass
    reduce_in_lib, torch_reduce, reduce_name = False, None, "none (1 GPU)"
    coll_dev = "cpu" if shared_devices else "cuda"    # where the tensors of this script's own collectives live
    rccl_path = None
    try:   # which librccl.so the library binds, and its version — at every N, so that the first 8-rank run is diagnosable from the line alone
        import ctypes
        rccl_path = lib.comm_library()
        ver = ctypes.c_int(0)
        if rccl_path and ctypes.CDLL(rccl_path).ncclGetVersion(ctypes.byref(ver)) == 0:
            rccl_path = "%s (ncclGetVersion %d)" % (rccl_path, ver.value)
    except Exception as e:  # noqa: BLE001
        rccl_path = "unavailable: %s" % e
    if world > 1:
        import datetime
        if shared_devices:
            # (gloo announces its peers on STDOUT; this script's stdout carries exactly one JSON line, so the announcement goes to stderr)
            sys.stdout.flush()
            saved_out = os.dup(1)
            os.dup2(2, 1)
            try:
                dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=600))
                dist.barrier()
            finally:
                sys.stdout.flush()
                os.dup2(saved_out, 1)
                os.close(saved_out)
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index), timeout=datetime.timedelta(seconds=600))
        # X1 lives in the library: rank 0's id travels over the launcher's process group, then every rank joins the library's own communicator
        try:
            uid = torch.zeros(128, dtype=torch.uint8, device=coll_dev)
            if rank == 0:
                uid.copy_(torch.frombuffer(bytearray(lib.comm_unique_id()), dtype=torch.uint8))
            dist.broadcast(uid, src=0)
            if shared_devices:
                raise RuntimeError("%d ranks on %d device(s): RCCL takes one rank per device" % (world, n_dev))
            lib.comm_init(rank, world, bytes(uid.cpu().numpy().tobytes()))
            ok = torch.ones(1, device=coll_dev)
        except Exception as e:  # noqa: BLE001 — a node without a usable librccl still gets its number through torch's communicator
            sys.stderr.write("rank %d: no library communicator (%s); the films are summed by torch.distributed.reduce\n" % (rank, e))
            ok = torch.zeros(1, device=coll_dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if ok.item() > 0:
            reduce_in_lib, reduce_name = True, "ncclReduce(sum) to rank 0 inside rspt_render_device (RCCL, library-owned communicator)"
        elif shared_devices:
            stage = torch.zeros(1, dtype=torch.float32).pin_memory()

            def torch_reduce(f):
                nonlocal stage
                torch.cuda.synchronize()  # the film was written on the library's stream
                if stage.numel() != f.numel():
                    stage = torch.zeros(f.numel(), dtype=torch.float32).pin_memory()
                stage.copy_(f)
                multigpu.reduce_film(stage)
                if rank == 0:
                    f.copy_(stage)
                torch.cuda.synchronize()
            reduce_name = "torch.distributed.reduce(sum) to rank 0 over gloo through host memory (%d ranks share %d device(s): RCCL takes one rank per device)" % (world, n_dev)
        else:
            def torch_reduce(f):
                torch.cuda.synchronize()  # the film was written on the library's stream
                multigpu.reduce_film(f)
                torch.cuda.synchronize()
            reduce_name = "torch.distributed.reduce(sum) to rank 0 (fallback: the library's RCCL communicator could not be created)"

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    shard = multigpu.shard_for_rank(rank, world)  # Morton-ordered tiles dealt round-robin over the ranks
    m = measure(args, lib, scenes, args.workload, args.steps, args.warmup, shard, world, reduce_in_lib, torch_reduce, fence, rank0=rank == 0)
    elapsed, stats = m["elapsed"], m["stats"]
    m_film_host = m["film_host"]
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        samples_t = torch.tensor([float(stats[0]["samples"])], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(samples_t, op=dist.ReduceOp.SUM)
        samples_per_step = float(samples_t.item())
    else:
        samples_per_step = float(stats[0]["samples"])

    if rank == 0:
        default_cfg = args.tris == 1_000_000 and not args.alpha_mask and not args.moving and args.filter == "box" and not args.res and not args.spp and world == 1 and args.integrator == "path" and args.sampler == "sobol"
        ms_per_step = elapsed / args.steps * 1e3
        if args.full:
            traffic, tnote, stale = measured_traffic(lib, args.workload, default_cfg)
            roofline = roofline_block(m["counts"], m["count_scale"], stats, traffic, tnote, stale, ms_per_step) if (m["counts"] and stats[0]["launches_closest"] + stats[0]["launches_any"] > 0) else (
                {"bound": "latency", "kernel": "k_tile_serial (one lane per tile: camera sample, reference-order traversal and shade_path in turn)", "achieved": None, "peak": None,
                 "unit": None, "frac": None, "traffic": None,
                 "note": "the pixel samplers make a tile one serial chain (DESIGN.md section 5.7): the bound is the dependent-load latency of one lane, "
                         "not bandwidth or issue rate; what is reported is the rate next to the CPU's"} if args.sampler not in ("sobol", "halton") else
                {"bound": "latency", "kernel": "k_lane_dl (DirectLightingIntegrator::li, one lane per camera sample: the specular tree, its light estimates and the texture stage in one kernel)",
                 "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None,
                 "note": "the per-lane form of directlighting (DESIGN.md section 5.4: textured materials / max_depth > 8 / several specular lobes of one kind); "
                         "no separate trace launches, the reference-order traversal runs inside the lane"})
        else:
            roofline = {"bound": None, "kernel": None, "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None,
                        "note": "not measured: the roofline needs a counting pass of its own, which only `bench.py --full` makes"}
        out = {
            "metric": "Mpath-samples/sec (whole node)", "value": samples_per_step * args.steps / elapsed / 1e6, "unit": "Msamples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": m["name"], "samples_per_step": samples_per_step, "tiles": "16x16 tiles in Morton order dealt round-robin to the ranks (tile_chunk %d)" % multigpu.TILE_CHUNK,
                       "film_reduce": reduce_name, "librccl": rccl_path, "devices_visible": n_dev,
                       "timed_region": "per step: rspt_render_device (first launch -> film complete in HBM%s) + the copy of the film to pinned host memory "
                                       "(%.1f MB): SURVEY 8(d)'s t_render, first launch -> film in host memory" % (
                                           " on rank 0 after the reduce" if world > 1 else "", scenes.n_pixels(m["rd"]) * 16 / 1e6)},
            "roofline": roofline,
            "stats": {k: sum(s_[k] for s_ in stats) / len(stats) for k in ("t_trace_closest_s", "t_trace_any_s", "t_trace_s", "t_shade_s", "t_kernels_s", "trace_launches", "truncated_paths", "nan_samples")},
            "setup_s": {"scene_and_bvh_build": m["t_scene"], "upload": m["t_upload"], "bvh_builder": "rspt_bvh_build_gpu (device, bit-identical to BVHAccel::new)"},
        }
        if args.workload == "cornell_docs" and not args.res and not args.spp and world == 1 and args.integrator == "path" and args.sampler == "sobol":
            out["vs_baseline"] = out["value"] / PUBLISHED_CORNELL_MSAMPLES
            out["baseline"] = ("%.2f Msamples/s = 500 * 500 * 8 samples / (1024 tiles / 1828.38 tiles/s): the reference's console transcript of this very render on 28 threads of an unnamed CPU "
                               "(docs/source/getting_started.rst:161-175; BASELINE.md section 1) — the only rate the reference publishes" % PUBLISHED_CORNELL_MSAMPLES)
        pyoracle = None
        if world == 1 and args.full and not args.no_cpu_baseline:  # the CPU baseline is reported on rank 0 at N = 1 only
            from oracle import pyoracle  # CPU baseline leg only
            rd0 = m["rd"]
            cx, cy = (rd0.crop_px[0] + rd0.crop_px[2]) // 2, (rd0.crop_px[1] + rd0.crop_px[3]) // 2
            fx, fy = float(rd0.full_res[0]), float(rd0.full_res[1])
            out["cpu_baseline"] = cpu_baseline(args, pyoracle, m["sc"], m["mk_rd"], args.cpu_spp, ((cx - 128) / fx, (cx + 128) / fx, (cy - 128) / fy, (cy + 128) / fy))
        if world == 1 and args.full and not args.no_extra and args.workload == "soup1m" and default_cfg:
            extra = {}
            # what the ranks of an 8-GPU node render: every shard (r, 8, tile_chunk) of the same frame on this one GPU, same kernels, no reduce;
            # the slowest shard bounds the 8-GPU frame time (static deal of interleaved Morton chunks: how even is it?)
            shard_ms = []
            for r in range(8):
                rd8 = m["mk_rd"](m["spp"], multigpu.shard_for_rank(r, 8))
                if r == 0:
                    lib.render_device(m["ds"], rd8, m["film"].data_ptr())  # warm-up (allocations sized for the shard)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st8 = [lib.render_device(m["ds"], rd8, m["film"].data_ptr()) for _ in range(args.steps)]
                torch.cuda.synchronize()
                shard_ms.append((time.perf_counter() - t0) / args.steps * 1e3)
            t1 = elapsed / args.steps * 1e3
            extra["eighth_frame_probe"] = {"ms": shard_ms[0], "samples": st8[0]["samples"], "full_frame_ms": t1, "shard_ms": shard_ms,
                                           "predicted_8gpu_speedup_before_reduce": t1 / max(shard_ms),
                                           "imbalance_max_over_mean": max(shard_ms) / (sum(shard_ms) / 8),
                                           "note": "one GPU rendering each shard (r, 8, tile_chunk) of the headline frame in turn: per-rank times of an 8-GPU run without the 16.8 MB reduce"}
            m["ds"].close()
            del m
            # C3: the north-star configuration (>= 100x CPU on the 4.3 M-triangle scene), timed by the same harness
            C3_STEPS = args.steps
            m3 = measure(args, lib, scenes, "statue", C3_STEPS, 1, (0, 1, 64), 1, False, None, fence, count_spp_div=16)
            s3 = float(m3["stats"][0]["samples"])
            c3 = {"metric": "Mpath-samples/sec", "value": s3 * C3_STEPS / m3["elapsed"] / 1e6, "unit": "Msamples/s", "steps": C3_STEPS, "warmup": 1,
                  "ms_per_step": m3["elapsed"] / C3_STEPS * 1e3, "config": {"workload": m3["name"], "samples_per_step": s3},
                  "roofline": roofline_block(m3["counts"], m3["count_scale"], m3["stats"], *measured_traffic(lib, "statue", True), m3["elapsed"] / C3_STEPS * 1e3),
                  "setup_s": {"scene_and_bvh_build": m3["t_scene"], "upload": m3["t_upload"]}}
            c3["roofline"]["counting_pass"] = "reference-order counters at 1/16 of the spp, scaled (per-sample means; SURVEY 8(d))"
            if pyoracle is not None:
                c3["cpu_baseline"] = cpu_baseline(args, pyoracle, m3["sc"], m3["mk_rd"], args.cpu_spp, (832 / 1920, 1088 / 1920, 412 / 1080, 668 / 1080))
                c3["gpu_over_cpu"] = c3["value"] / c3["cpu_baseline"]["value"]
            extra["c3_statue_standin"] = c3
            m3["ds"].close()
            out["extra"] = extra
            # the driver's parser keeps `config` and `roofline` whole and only the key names of `extra`: the north-star scene's stand-in and the
            # shard probe ride in `config` as flat summaries; the full blocks stay in `extra`
            out["config"]["c3_statue_standin"] = {"workload": m3["name"], "value_msamples_s": c3["value"], "ms_per_step": c3["ms_per_step"], "steps": C3_STEPS,
                                                  "roofline_frac": c3["roofline"].get("frac"), "binding_frac": c3["roofline"].get("binding_frac"),
                                                  "shade_frac": c3["roofline"]["shade"].get("frac"), "shade_s": c3["roofline"]["shade"].get("seconds_per_step"),
                                                  "shade_traffic_over_algorithmic": c3["roofline"]["shade"].get("traffic_over_algorithmic"),
                                                  "cpu_baseline_msamples_s": c3.get("cpu_baseline", {}).get("value"), "cpu_cores": c3.get("cpu_baseline", {}).get("cores"),
                                                  "gpu_over_cpu": c3.get("gpu_over_cpu"), "note": "a declared stand-in for BASELINE configs[2] (the Ganesha PLY is not in the image)"}
            out["config"]["eighth_frame_probe"] = {"shard_ms_max": max(shard_ms), "shard_ms_mean": sum(shard_ms) / 8, "full_frame_ms": t1,
                                                   "predicted_8gpu_speedup_before_reduce": t1 / max(shard_ms)}
        if shared_devices:
            out["config"]["note"] = ("%d ranks on %d device(s): a run of the N > 1 CONTROL FLOW (spawn, id exchange, tile deal, film sum, max-over-ranks timing), "
                                     "not a scaling measurement" % (world, n_dev))
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, m_film_host.numpy().reshape(-1, 4))
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        if reduce_in_lib:
            lib.comm_destroy()
        dist.destroy_process_group()
    if args.watchdog > 0:
        faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
