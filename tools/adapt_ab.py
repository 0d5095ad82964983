"""Interleaved timing, in ONE process, of adaptive accumulation (rt_adapt_*,
DESIGN.md 5.7) against the plain accumulator of the same build (tools/ab.py's
method: host clock around a stream synchronise).

  python tools/adapt_ab.py [--config c2] [--rounds 9] [--reps 1] [--spp 64] [--pass 4]
                           [--tolerance T --bias B --min-samples M] [--lib path/to/libraytracer.so]

Every round times, for each variant in turn, `reps` repetitions after one
untimed repetition of the same variant, of a whole accumulation of spp samples
in passes of `pass` (rt_accum_reset first; the first pass zero-fills the planes):
  plain            the plain accumulator, passes only enqueued, one wait at the end
  plain_synced     the same with a stream synchronise after every pass (what an
                   adaptive pass's length readback costs a plain one)
  adapt_full       adaptive with min_samples > spp: every pixel stays listed, no
                   decision -- the cost of the list indirection, the fourth fold
                   and the count kernel at 100 % active
  adapt_decide     adaptive with tolerance 0, bias 0: a decision (select,
                   compact, readback) after every pass from min_samples on, yet
                   only pixels without variance leave
  adapt            adaptive at the given options (default: the library's), until
                   the list is empty or spp is reached
and prints one JSON line per variant: median / min / max ms per repetition over
the rounds and the ratio of medians to plain.  For the synced and adaptive
variants it adds per pass the median ms, and for `adapt` the active share
before the pass and the samples it traced, plus the totals.  plain_synced and
adapt_full must give plain's frame (checked before any timing).
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
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--pass", dest="n", type=int, default=4)
    ap.add_argument("--tolerance", type=float, default=None)
    ap.add_argument("--bias", type=float, default=None)
    ap.add_argument("--min-samples", type=int, default=None)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    make_scene, W, H, spp, depth = S.CONFIGS[args.config]
    spp = args.spp or spp
    n = args.n
    assert spp % n == 0, "the pass size must divide spp"
    npass = spp // n
    torch.cuda.set_device(0)
    world = R.World(make_scene(), lib_path=args.lib)
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    outs = {}

    def accumulator(label, **adaptive):
        acc = world.accumulator(W, H, spp, depth=depth, device=0)
        if adaptive:
            acc.set_adaptive(**adaptive)
        outs[label] = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
        return acc

    accs = {
        "plain": accumulator("plain"),
        "plain_synced": accumulator("plain_synced"),
        "adapt_full": accumulator("adapt_full", min_samples=spp + 1),
        "adapt_decide": accumulator("adapt_decide", tolerance=0.0, bias=0.0),
        "adapt": accumulator("adapt", tolerance=args.tolerance, bias=args.bias, min_samples=args.min_samples),
    }
    per_pass = {k: [] for k in accs if k != "plain"}   # per repetition: [ms per pass]
    shares, traced = [], []                            # adapt: per repetition, per pass

    def run(label, record):
        acc, out = accs[label], outs[label]
        acc.reset()
        synced = label != "plain"
        ms, sh, tr = [], [], []
        for _ in range(npass):
            active = acc.active if label == "adapt" else W * H
            if active == 0:
                break
            t = time.perf_counter()
            acc.add_device(n, out.data_ptr(), sp)
            if synced:
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t) * 1e3)
            sh.append(active / (W * H))
            tr.append(active * n)
        torch.cuda.synchronize()
        if record and synced:
            per_pass[label].append(ms)
            if label == "adapt":
                shares.append(sh)
                traced.append(tr)

    for label in accs:
        run(label, False)
    torch.cuda.synchronize()
    for label in ("plain_synced", "adapt_full"):
        assert torch.equal(outs["plain"], outs[label]), f"{label}: frame differs from the plain accumulator's"

    res = {label: [] for label in accs}
    for rnd in range(args.rounds + 1):
        for label in accs:
            run(label, False)  # (untimed: the measurement's predecessor is the variant itself)
            t = time.perf_counter()
            for _ in range(args.reps):
                run(label, rnd > 0)
            if rnd:  # (round 0 warms up)
                res[label].append((time.perf_counter() - t) * 1e3 / args.reps)
    base = statistics.median(res["plain"])
    for label in accs:
        r = res[label]
        line = {"variant": label, "config": args.config, "width": W, "height": H, "spp": spp, "pass": n,
                "rounds": args.rounds, "reps": args.reps, "ms_median": statistics.median(r), "ms_min": min(r),
                "ms_max": max(r), "vs_plain_median": statistics.median(r) / base}
        if label in per_pass:
            rows = per_pass[label]
            k = min(len(x) for x in rows)
            line["passes"] = k
            line["pass_ms_median"] = [round(statistics.median(x[i] for x in rows), 4) for i in range(k)]
            line["pass_ms_min"] = [round(min(x[i] for x in rows), 4) for i in range(k)]
            line["pass_ms_max"] = [round(max(x[i] for x in rows), 4) for i in range(k)]
        if label == "adapt":
            o = R.AdaptOptions()
            R.lib(args.lib).rt_adapt_default_options(o)
            line["tolerance"] = args.tolerance if args.tolerance is not None else float(o.tolerance)
            line["bias"] = args.bias if args.bias is not None else float(o.bias)
            line["min_samples"] = args.min_samples if args.min_samples is not None else int(o.min_samples)
            line["active_share_before_pass"] = [round(x, 4) for x in shares[0]]
            line["samples_traced"] = traced[0]
            line["samples_traced_total"] = sum(traced[0])
            line["samples_plain_total"] = W * H * spp
            line["active_at_end"] = accs["adapt"].active
            assert all(s == shares[0] for s in shares), "the list is not the same in every repetition"
        print(json.dumps(line))


if __name__ == "__main__":
    main()
