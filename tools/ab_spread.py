"""tools/ab.py's interleaved lean-frame timing with every round kept: one JSON
line per variant with each round's lean-frame ms, their median, min, max and
spread (max - min), and the counting frame's BVH counters and tree layout.
A gain counts when it exceeds twice the baseline's own spread.

  python tools/ab_spread.py --variant new=rust-swift-raytracer_amd/lib/libraytracer.so \\
         --variant parent=ab/parent/libraytracer.so \\
         --variant off=rust-swift-raytracer_amd/lib/libraytracer.so:RT_AMD_CORNER=0 \\
         [--config c2] [--rounds 9] [--frames 3]
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
    ap.add_argument("--variant", action="append", required=True)
    ap.add_argument("--config", default="c2")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=3)
    args = ap.parse_args()
    make_scene, W, H, spp, depth = S.CONFIGS[args.config]
    src = make_scene()
    torch.cuda.set_device(0)
    out = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    variants = []
    for v in args.variant:
        label, rest = v.split("=", 1)
        parts = rest.split(":")
        path = os.path.join(ROOT, parts[0])
        env = dict(kv.split("=", 1) for kv in parts[1:])
        os.environ.update(env)
        variants.append((label, R.World(src, lib_path=path), env))
        for k in env:
            os.environ.pop(k, None)
    res = {label: [] for label, _, _ in variants}
    stats = {}
    for rnd in range(args.rounds + 1):
        for label, world, env in variants:
            os.environ.update(env)
            st = world.render_device(W, H, out.data_ptr(), stream.cuda_stream, spp=spp, depth=depth, device=0)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.frames):
                world.render_device(W, H, out.data_ptr(), stream.cuda_stream, spp=spp, depth=depth,
                                    device=0, stats=False)
            torch.cuda.synchronize()
            lean = (time.perf_counter() - t) * 1e3 / args.frames
            for k in env:
                os.environ.pop(k, None)
            if rnd:
                res[label].append(lean)
                stats[label] = st
    for label, r in res.items():
        st = stats[label]
        print(json.dumps({"variant": label, "config": args.config, "lean_ms": [round(x, 4) for x in r],
                          "median": statistics.median(r), "min": min(r), "max": max(r),
                          "spread": max(r) - min(r), "rays": st["rays"],
                          "bvh_node_tests": st["bvh_node_tests"], "bvh_sphere_tests": st["bvh_sphere_tests"],
                          "sphere_tree": st.get("sphere_tree"), "lds_bytes": st.get("sphere_tree_lds_bytes"),
                          "blocks": st["launch_blocks"], "threads": st["launch_block_threads"]}))


if __name__ == "__main__":
    main()
