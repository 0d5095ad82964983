"""Interleaved timing, in ONE process, of the primary triangle strip lists built
on the device against the host build (RT_AMD_GPU_TRI_LISTS 1 against 0; read
per frame, so one world serves both), in tools/accum_ab.py's manner.

  python tools/lists_ab.py [--config c5] [--rounds 7] [--reps 3] [--spp 64]

What a viewer waits for after a mouse-look step: the camera turns in place by
1 degree (same origin: the camera-origin records stay, the lists are rebuilt),
then the first picture, host wait included.  Every round times, for each
setting in turn, `reps` repetitions after one untimed repetition of the same
variant, of
  turn_pass1    turn, one accumulator pass of 1 sample, stream synchronise
  turn_frame    turn, the one-shot frame at spp samples, stream synchronise
  steady_pass1  a pass of 1 without a turn (lists reused)
  steady_frame  the one-shot frame without a turn
and prints one JSON line per (variant, setting): median / min / max ms over
the rounds.  A last line per turn variant says whether the device build's
median is below the host build's by more than twice the host leg's min-max
spread (DESIGN.md 9's bar for a default).  Before any timing the two settings'
frames are compared (same bits) and rt_primary_tri_lists must report 1 and 2.
"""
import argparse
import json
import math
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

KNOB = "RT_AMD_GPU_TRI_LISTS"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=0)
    args = ap.parse_args()
    make_scene, W, H, spp, depth = S.CONFIGS[args.config]
    spp = args.spp or spp
    torch.cuda.set_device(0)
    world = R.World(make_scene())
    cam = world.camera()
    origin = cam[0:3].copy()
    aspect = float(cam[6] / cam[10])
    vfov = 2.0 * math.atan(float(cam[10]) / 2.0)  # the scene camera: viewport height at focal length 1
    acc = world.accumulator(W, H, spp, depth=depth, device=0)
    out = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    step = [0]

    def turn():  # 1 degree per call, swinging between -5 and +5 degrees about the y axis
        step[0] += 1
        a = math.radians(abs(step[0] % 20 - 10) - 5)
        world.look_at(origin, (origin[0] + math.sin(a), origin[1], origin[2] - math.cos(a)), (0, 1, 0), vfov, aspect)

    def pass1():
        if acc.samples >= spp:
            acc.reset()
        acc.add_device(1, out.data_ptr(), sp)
        torch.cuda.synchronize()

    def frame():
        world.render_device(W, H, out.data_ptr(), sp, spp=spp, depth=depth, device=0, stats=False)
        torch.cuda.synchronize()

    def turn_pass1():
        turn()
        pass1()

    def turn_frame():
        turn()
        frame()

    # the same frame from both settings, built where the knob says, before anything is timed
    frames = {}
    for setting in ("0", "1"):
        os.environ[KNOB] = setting
        turn()
        step[0] -= 1  # (the same camera for both)
        frame()
        assert world.primary_tri_lists(0) == 1 + int(setting), (setting, world.primary_tri_lists(0))
        frames[setting] = out.clone()
        world.look_at(origin, (origin[0], origin[1], origin[2] - 1.0), (0, 1, 0), vfov, aspect)
        frame()  # (another camera in between: the next setting rebuilds)
    assert torch.equal(frames["0"], frames["1"]), "host-built and device-built lists give different frames"

    variants = [("turn_pass1", turn_pass1), ("turn_frame", turn_frame), ("steady_pass1", pass1),
                ("steady_frame", frame)]
    res = {(label, s): [] for label, _ in variants for s in ("0", "1")}
    for rnd in range(args.rounds + 1):
        for label, fn in variants:
            for setting in ("0", "1"):
                os.environ[KNOB] = setting
                fn()  # (untimed: the measurement's predecessor is the variant itself)
                t = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                if rnd:  # (round 0 warms up)
                    res[label, setting].append((time.perf_counter() - t) * 1e3 / args.reps)
    for (label, setting), r in res.items():
        print(json.dumps({"variant": label, KNOB: int(setting), "config": args.config, "width": W, "height": H,
                          "spp": 1 if "pass1" in label else spp, "rounds": args.rounds, "reps": args.reps,
                          "ms_median": statistics.median(r), "ms_min": min(r), "ms_max": max(r)}))
    for label in ("turn_pass1", "turn_frame"):
        host, dev = res[label, "0"], res[label, "1"]
        gain = statistics.median(host) - statistics.median(dev)
        spread = max(host) - min(host)
        print(json.dumps({"variant": label, "host_minus_device_ms": gain, "host_spread_ms": spread,
                          "device_build_accepted": gain > 2 * spread}))


if __name__ == "__main__":
    main()
