"""Do a frame's sky kernel and its trace launch overlap?  Reads the kernel trace
of one `rocprofv3 --kernel-trace --stats --output-format csv` run (the
*_kernel_trace.csv) and pairs every sky_rows_kernel dispatch with its frame's
trace_kernel dispatch: the next trace dispatch (--sky first: the one-stream
order, sky kernel in front) or the one before (--sky last: the forked order,
sky kernel enqueued behind the trace launch).  Prints one JSON line: medians
over the pairs, in microseconds, of both durations, the overlap (how long both
ran), the gap (start of the later minus end of the earlier, negative when they
overlap), the span (first start to last end) and the two durations added; and
the queues the two kernels ran on.

  python tools/sky_fork_overlap.py trace/new_kernel_trace.csv --sky last
"""
import argparse
import csv
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--sky", choices=["first", "last"], required=True)
    args = ap.parse_args()
    with open(args.csv, newline="") as fh:
        rows = [r for r in csv.DictReader(fh)]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    ks = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"))
          for r in rows if "sky_rows_kernel" in r["Kernel_Name"] or "trace_kernel" in r["Kernel_Name"]]
    pairs = []
    for i, k in enumerate(ks):
        if "sky_rows_kernel" not in k[0]:
            continue
        j = i + 1 if args.sky == "first" else i - 1
        if 0 <= j < len(ks) and "trace_kernel" in ks[j][0]:
            pairs.append((k, ks[j]))
    if not pairs:
        raise SystemExit("no sky kernel with a trace launch next to it in this trace")
    med = lambda f: round(statistics.median(f(s, t) for s, t in pairs) / 1e3, 2)  # noqa: E731
    print(json.dumps({
        "csv": args.csv, "sky": args.sky, "pairs": len(pairs),
        "sky_us": med(lambda s, t: s[2] - s[1]),
        "trace_us": med(lambda s, t: t[2] - t[1]),
        "overlap_us": med(lambda s, t: max(0, min(s[2], t[2]) - max(s[1], t[1]))),
        "gap_us": med(lambda s, t: max(s[1], t[1]) - min(s[2], t[2])),
        "span_us": med(lambda s, t: max(s[2], t[2]) - min(s[1], t[1])),
        "added_us": med(lambda s, t: (s[2] - s[1]) + (t[2] - t[1])),
        "sky_starts_before_trace_ends": sum(1 for s, t in pairs if s[1] < t[2] and t[1] < s[2]),
        "sky_queues": sorted({s[3] for s, _ in pairs}), "trace_queues": sorted({t[3] for _, t in pairs}),
        "last_pair": {"sky": list(pairs[-1][0][1:3]), "trace": list(pairs[-1][1][1:3])},
    }))


if __name__ == "__main__":
    main()
