"""Interleaved timing, in ONE process, of progressive accumulation against the
lean one-shot frame of the same build (tools/ab.py's method: enqueued frames
without stats, host clock around a stream synchronise).

  python tools/accum_ab.py [--config c2] [--rounds 9] [--reps 3] [--spp 64]
                           [--splits 1,4,64] [--lib path/to/libraytracer.so]

Every round times, for each variant in turn, `reps` back-to-back repetitions
after one untimed repetition of the same variant (what ran just before a
measurement moves it by several percent; this way every variant follows
itself), of
  lean        the one-shot frame at spp samples per pixel (rt_render_device)
  accum_KxN   a whole accumulation of spp samples as K passes of N = spp / K
              (rt_accum_reset, then K rt_accum_add_device; the first pass
              zero-fills the sum planes)
  accum_pass_of_1_synced   one pass of 1 sample followed by a stream
              synchronise (what a viewer's redraw waits for)
and prints one JSON line per variant: median / min / max ms per repetition
over the rounds (the spread), the ratio of medians to lean, and for the
accumulations the ms per pass.  The final frames are compared with the
one-shot frame (same bits) before any timing.
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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--splits", default="1,4,64", help="pass counts K (each must divide spp)")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    make_scene, W, H, spp, depth = S.CONFIGS[args.config]
    spp = args.spp or spp
    splits = [int(k) for k in args.splits.split(",")]
    assert all(spp % k == 0 for k in splits), "every pass count must divide spp"
    torch.cuda.set_device(0)
    world = R.World(make_scene(), lib_path=args.lib)
    acc = world.accumulator(W, H, spp, depth=depth, device=0)
    out = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    out2 = torch.zeros_like(out)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream

    def lean():
        world.render_device(W, H, out.data_ptr(), sp, spp=spp, depth=depth, device=0, stats=False)

    def accum(k):
        acc.reset()
        for _ in range(k):
            acc.add_device(spp // k, out2.data_ptr(), sp)

    # the same frame, whatever the split, before anything is timed
    lean()
    for k in splits:
        accum(k)
        torch.cuda.synchronize()
        assert torch.equal(out, out2), f"{k} passes of {spp // k}: frame differs from the one-shot frame"
    def one_synced():  # what a viewer's redraw waits for: one pass of 1 sample, host wait included
        if acc.samples >= spp:
            acc.reset()
        acc.add_device(1, out2.data_ptr(), sp)
        torch.cuda.synchronize()

    variants = [("lean", lean)] + [(f"accum_{k}x{spp // k}", (lambda k=k: accum(k))) for k in splits]
    variants.append(("accum_pass_of_1_synced", one_synced))
    splits = splits + [1]
    res = {label: [] for label, _ in variants}
    for rnd in range(args.rounds + 1):
        for label, fn in variants:
            fn()  # (untimed: the measurement's predecessor is the variant itself)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            if rnd:  # (round 0 warms up)
                res[label].append((time.perf_counter() - t) * 1e3 / args.reps)
    base = statistics.median(res["lean"])
    for (label, _), k in zip(variants, [0] + splits):
        r = res[label]
        line = {"variant": label, "config": args.config, "width": W, "height": H, "spp": spp, "rounds": args.rounds,
                "reps": args.reps, "ms_median": statistics.median(r), "ms_min": min(r), "ms_max": max(r),
                "vs_lean_median": statistics.median(r) / base}
        if k:
            line["passes"] = k
            line["ms_per_pass_median"] = statistics.median(r) / k
        print(json.dumps(line))


if __name__ == "__main__":
    main()
