"""Interleaved timing, in ONE process, of the first-hit calls against the
cheapest thing the library could do for the same pixels before them: an
accumulation pass of 1 sample with max_ray_bounces = 1 (tools/accum_ab.py's
method: enqueued calls, host clock around a stream synchronise).

  python tools/first_hit_ab.py [--config c2] [--rounds 12] [--reps 5] [--picks 200]
                               [--lib path/to/libraytracer.so]

Every round times, for each leg in turn, `reps` back-to-back repetitions after
one untimed repetition of the same leg (every leg follows itself), of
  accum_pass_1_depth_1    one accumulation pass of 1 sample, depth 1 (rt_accum_add_device)
  first_hit_device        the 32-byte records of the whole frame (rt_first_hit_device)
  first_hit_view_normal   the RT_VIEW_NORMAL frame (rt_first_hit_view_device)
and prints one JSON line per leg: median / min / max ms per repetition over the
rounds, the ratio of medians to the baseline, and whether the leg's median is
above the baseline's by no more than the baseline's own min-max spread in this
run (DESIGN.md 5.8's expectation).  A last line is the latency of one
rt_first_hit_pick with its host wait (median / min / max over --picks calls at
seeded pixels).  BRUTE and BVH records are compared (same bytes) before timing.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-swift-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import raytracer_amd as R  # noqa: E402
import scenes as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--picks", type=int, default=200)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    assert args.rounds >= 12, "at least 12 rounds"
    make_scene, W, H, _spp, _depth = S.CONFIGS[args.config]
    torch.cuda.set_device(0)
    world = R.World(make_scene(), lib_path=args.lib)
    # (a stride no run reaches: the accumulator never resets inside a measurement)
    stride = (args.rounds + 1) * (args.reps + 1) + 1
    acc = world.accumulator(W, H, stride, depth=1, device=0)
    rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    view = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    rec2 = torch.zeros_like(rec)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream

    # the same records from both searches, before anything is timed (small scenes only:
    # brute force over 100,000 triangles per pixel is minutes)
    if world.num_triangles <= 1000:
        world.first_hit_device(W, H, rec.data_ptr(), sp, accel=R.ACCEL_BRUTE, device=0)
        world.first_hit_device(W, H, rec2.data_ptr(), sp, accel=R.ACCEL_BVH, device=0)
        torch.cuda.synchronize()
        assert torch.equal(rec, rec2), "BRUTE and BVH records differ"

    legs = [
        ("accum_pass_1_depth_1", lambda: acc.add_device(1, rgba.data_ptr(), sp)),
        ("first_hit_device", lambda: world.first_hit_device(W, H, rec.data_ptr(), sp, device=0)),
        ("first_hit_view_normal", lambda: world.first_hit_view_device(W, H, R.VIEW_NORMAL, view.data_ptr(), sp, device=0)),
    ]
    res = {label: [] for label, _ in legs}
    for rnd in range(args.rounds + 1):
        for label, fn in legs:
            fn()  # (untimed: the measurement's predecessor is the leg itself)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            if rnd:  # (round 0 warms up)
                res[label].append((time.perf_counter() - t) * 1e3 / args.reps)
    base = res[legs[0][0]]
    base_med, base_spread = statistics.median(base), max(base) - min(base)
    for label, _ in legs:
        r = res[label]
        med = statistics.median(r)
        print(json.dumps({"leg": label, "config": args.config, "width": W, "height": H, "rounds": args.rounds,
                          "reps": args.reps, "ms_median": med, "ms_min": min(r), "ms_max": max(r),
                          "vs_baseline_median": med / base_med, "baseline_spread_ms": base_spread,
                          "within_baseline_spread": bool(med - base_med <= base_spread)}))

    # one pick with its host wait: what an editor's click costs
    rng = np.random.default_rng(1)
    pts = [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(args.picks + 8)]
    lat, hits = [], 0
    for k, (col, row) in enumerate(pts):
        t = time.perf_counter()
        r = world.pick(W, H, col, row, device=0)
        dt = (time.perf_counter() - t) * 1e3
        if k >= 8:  # (the first ones warm up)
            lat.append(dt)
            hits += int(r["prim"] != 0)
    print(json.dumps({"leg": "first_hit_pick_latency", "config": args.config, "width": W, "height": H,
                      "picks": len(lat), "hits": hits, "ms_median": statistics.median(lat), "ms_min": min(lat),
                      "ms_max": max(lat)}))


if __name__ == "__main__":
    main()
