"""Interleaved timing, in ONE process, of the history resolve with its
neighbourhood clamp (rt_clamp_enable) against the unclamped
resolve and a one-level filter of the same accumulator (tools/history_ab.py's
method: enqueued calls, host clock around a stream synchronise).

  python tools/clamp_ab.py [--config c2] [--rounds 12] [--reps 3] [--lib path/to/libraytracer.so]

Every round times, for each leg in turn, `reps` back-to-back repetitions after
one untimed repetition of the same leg (every leg follows itself), of
  filter_levels_1        rt_filter_accum_device at levels = 1, records cached
  resolve_unclamped      rt_history_resolve_device, no filter, prev valid, records cached
  resolve_clamp_r1       the same with the clamp at radius 1 (9 taps)
  resolve_clamp_r3       the same with the clamp at radius 3 (49 taps)
and prints one JSON line per leg: median / min / max ms per repetition over the
rounds, the ratio of medians to the one-level filter, and whether the leg's
median is above that filter's by no more than the filter's own min-max spread in
this run (DESIGN.md 5.10a's expectation, which is about resolve_clamp_r1).  The
clamp's setting is switched between the legs, outside the timed calls: it is a
host-side field.
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

import torch  # noqa: E402

import raytracer_amd as R  # noqa: E402
import scenes as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    assert args.rounds >= 12, "at least 12 rounds"
    make_scene, W, H, _spp, _depth = S.CONFIGS[args.config]
    torch.cuda.set_device(0)
    world = R.World(make_scene(), lib_path=args.lib)
    acc = world.accumulator(W, H, 64, device=0)
    acc.history_enable()
    rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    px = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream

    def resolve():
        acc.resolved_device(out.data_ptr(), px.data_ptr(), sp)

    # a resolved view behind the current one: prev is valid from here on
    acc.add_device(4, rgba.data_ptr(), sp)
    resolve()
    world.translate_camera(0.01, 0.0, 0.0)
    acc.add_device(1, rgba.data_ptr(), sp)
    resolve()
    torch.cuda.synchronize()

    def timed(fn, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    def clamped(radius):
        def leg(reps):
            acc.clamp_enable(radius=radius)
            return timed(resolve, reps)
        return leg

    def unclamped(reps):
        acc.clamp_disable()
        return timed(resolve, reps)

    legs = [
        ("filter_levels_1", lambda reps: timed(lambda: acc.filtered_device(out.data_ptr(), px.data_ptr(), sp, levels=1),
                                               reps)),
        ("resolve_unclamped", unclamped),
        ("resolve_clamp_r1", clamped(1)),
        ("resolve_clamp_r3", clamped(3)),
    ]
    res = {label: [] for label, _ in legs}
    for rnd in range(args.rounds + 1):
        for label, fn in legs:
            fn(1)  # (untimed: the measurement's predecessor is the leg itself)
            ms = fn(args.reps)
            if rnd:  # (round 0 warms up)
                res[label].append(ms)
    assert float(acc.history_length().max()) > acc.samples, "prev was not valid: nothing was reprojected"
    base = res[legs[0][0]]
    base_med, base_spread = statistics.median(base), max(base) - min(base)
    for label, _ in legs:
        r = res[label]
        med = statistics.median(r)
        print(json.dumps({"leg": label, "config": args.config, "width": W, "height": H, "rounds": args.rounds,
                          "reps": args.reps, "ms_median": med, "ms_min": min(r), "ms_max": max(r),
                          "vs_filter_median": med / base_med, "filter_spread_ms": base_spread,
                          "within_filter_spread": bool(med - base_med <= base_spread)}))


if __name__ == "__main__":
    main()
