#!/usr/bin/env python3
"""Times pg_scatter_sample_at against pg_intersect_at on the same device pointers in one process: rays aimed at BASELINE config 3's scene
(scenes/gen_synthetic.py), device memory, no interaction output; host clock around calls that end in the entry point's own synchronise, the two calls
alternating.  Prints one JSON line.  Run on the GPU box: python tools/scatter_timing.py [--rays N] [--grid G] [--reps R]
(under `rocprofv3 --kernel-trace --stats -- python tools/scatter_timing.py --reps 3` the kernels' own times: tools/kstats.py prints them)."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scenes"))
spec = importlib.util.spec_from_file_location("pbrt_v3_amd", os.path.join(ROOT, "pbrt-v3_amd", "__init__.py"), submodule_search_locations=[os.path.join(ROOT, "pbrt-v3_amd")])
pkg = importlib.util.module_from_spec(spec)
sys.modules["pbrt_v3_amd"] = pkg
spec.loader.exec_module(pkg)


def aimed_rays(scene, n, seed):
    """n rays from inside the upper half of the scene's bounds towards the centroids of random triangles."""
    rng = np.random.default_rng(seed)
    desc = scene.desc
    nodes = scene.nodes()
    lo, hi = nodes["bmin"][0], nodes["bmax"][0]
    ext = hi - lo
    idx = np.ctypeslib.as_array(desc.indices, (desc.n_tris, 3))[rng.integers(0, desc.n_tris, n)]
    P = np.ctypeslib.as_array(desc.P, (desc.n_verts, 3))
    c = (P[idx[:, 0]] + P[idx[:, 1]] + P[idx[:, 2]]) / np.float32(3)
    o = (lo + ext * (np.array([0.1, 0.1, 0.5]) + np.array([0.8, 0.8, 0.4]) * rng.random((n, 3)))).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray((c - o).astype(np.float32)), np.full(n, np.inf, np.float32), rng.random((n, 2)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, default=708, help="heightfield vertices per side (708: config 3, 999 698 triangles)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import gen_synthetic
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: a timing needs the device")
    with tempfile.TemporaryDirectory() as work:
        path = os.path.join(work, "synthetic.pbrt")
        gen_synthetic.write_scene(path, n=args.grid, xres=64, yres=64, spp=1)
        scene = pkg.HostScene(path)
    gs = pkg.GpuScene(scene.desc)
    n = args.rays
    o, d, tmax, u = aimed_rays(scene, n, 9)
    dev = [torch.from_numpy(a).cuda() for a in (o, d, tmax, u)]
    isect = torch.zeros(n * pkg.INTERACTION_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    scat = torch.zeros(n * pkg.SCATTER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    po, pd, pt, pu = (t.data_ptr() for t in dev)
    torch.cuda.synchronize()

    def call_scatter():
        gs.scatter_sample_at_device(n, po, pd, pt, None, pu, 31, None, scat.data_ptr())

    def call_intersect():
        gs.intersect_at_device(n, po, pd, pt, None, isect.data_ptr())

    times = {"pg_scatter_sample_at": [], "pg_intersect_at": []}
    trace_ms = {"pg_scatter_sample_at": [], "pg_intersect_at": []}
    for rep in range(args.warmup + args.reps):
        for name, call in (("pg_scatter_sample_at", call_scatter), ("pg_intersect_at", call_intersect)):
            before = gs.counters()["closest_ms"]
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            if rep >= args.warmup:
                times[name].append((t1 - t0) * 1e3)
                trace_ms[name].append(gs.counters()["closest_ms"] - before)
    rec = scat.cpu().numpy().view(pkg.SCATTER_DTYPE)
    it = isect.cpu().numpy().view(pkg.INTERACTION_DTYPE)
    out = {"rays": n, "triangles": int(scene.desc.n_tris), "reps": args.reps, "hit_fraction": round(float((rec["prim"] >= 0).mean()), 4),
           "sampled_fraction": round(float((rec["pdf"] != 0).mean()), 4), "same_prims": bool(np.array_equal(rec["prim"], it["prim"]))}
    for name in times:
        med = statistics.median(times[name])
        out[name] = {"median_ms": round(med, 3), "min_ms": round(min(times[name]), 3), "max_ms": round(max(times[name]), 3), "mrays_per_s": round(n / med / 1e3, 1),
                     "k_trace_median_ms": round(statistics.median(trace_ms[name]), 3)}
    print(json.dumps(out))
    gs.close()


if __name__ == "__main__":
    main()
