#!/usr/bin/env python3
"""What one timed step of bench.py puts on the stream, from a rocprofv3 --kernel-trace --memory-copy-trace run written
with --output-format csv: per step the solve launch, whatever follows it before the next solve launch (kernels and
memory copies, in stream order, each with the gap in front of it), and the step's period from launch start to launch
start.  Medians over the last --steps solve launches (the timed ones; the warm-up comes first).  Prints one JSON object.

usage: tools/step_trace_summary.py DIR [--steps 20] [--solve step_solve_face]     (DIR holds *_kernel_trace.csv)"""
import argparse
import csv
import glob
import json
import os
import statistics


def rows(pattern):
    out = []
    for f in glob.glob(pattern):
        out += list(csv.DictReader(open(f)))
    return out


def short(name):
    name = name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
    return name.split("::")[-1].replace("void ", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--solve", default="step_solve_face")
    a = ap.parse_args()
    ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in rows(os.path.join(a.dir, "*kernel_trace.csv"))]
    ev += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Direction"]) for r in rows(os.path.join(a.dir, "*memory_copy_trace.csv"))]
    ev.sort()
    at = [i for i, e in enumerate(ev) if a.solve in e[2]]
    at = at[-(a.steps + 1):]     # one more: the last timed step ends where the statistics launch begins or the list ends
    steps = []
    for k, i in enumerate(at[:a.steps] if len(at) > a.steps else at):
        j = at[k + 1] if k + 1 < len(at) else len(ev)
        seq, prev_end = [], ev[i][1]
        for s, e, name in ev[i + 1:j]:
            seq.append({"what": name, "gap_us": (s - prev_end) / 1e3, "us": (e - s) / 1e3})
            prev_end = e
        steps.append({"solve_us": (ev[i][1] - ev[i][0]) / 1e3, "solve": ev[i][2], "after": seq,
                      "period_us": (ev[j][0] - ev[i][0]) / 1e3 if j < len(ev) else None,
                      "gap_to_next_solve_us": (ev[j][0] - prev_end) / 1e3 if j < len(ev) else None})
    shapes = sorted({tuple(x["what"] for x in s["after"]) for s in steps})
    med = lambda v: statistics.median(v) if v else None
    out = {"steps": len(steps), "solve_kernel": steps[0]["solve"] if steps else None,
           "solve_us": {"median": med([s["solve_us"] for s in steps]), "min": min(s["solve_us"] for s in steps), "max": max(s["solve_us"] for s in steps)},
           "period_us_median": med([s["period_us"] for s in steps if s["period_us"]]),
           "gap_to_next_solve_us_median": med([s["gap_to_next_solve_us"] for s in steps if s["gap_to_next_solve_us"] is not None]),
           "after_the_solve": [list(x) for x in shapes]}
    common = max(shapes, key=lambda sh: sum(1 for s in steps if tuple(x["what"] for x in s["after"]) == sh)) if shapes else ()
    same = [s for s in steps if tuple(x["what"] for x in s["after"]) == common]
    out["after_the_solve_medians"] = [{"what": w, "gap_us": med([s["after"][n]["gap_us"] for s in same]), "us": med([s["after"][n]["us"] for s in same])}
                                      for n, w in enumerate(common)]
    out["outside_the_solve_us_median"] = med([s["period_us"] - s["solve_us"] for s in steps if s["period_us"]])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
