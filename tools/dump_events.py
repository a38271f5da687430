"""Print what a TensorBoard event file holds: per event the step and, per value, the tag with the scalar's value, the histogram's
num / min / max / non-empty buckets, or the image's size.  Both CRCs of every record are verified (phiseg_code_amd/summary.py).

    python tools/dump_events.py <log dir or events.out.tfevents.* file> [--tags-only]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phiseg_code_amd import summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--tags-only", action="store_true", help="one line per tag: kind, number of events, first and last step")
    args = ap.parse_args()
    paths = [args.path]
    if os.path.isdir(args.path):
        paths = sorted(os.path.join(args.path, f) for f in os.listdir(args.path) if f.startswith("events.out.tfevents."))
        if not paths:
            sys.exit("no events.out.tfevents.* file in %s" % args.path)
    for path in paths:
        print("== %s" % path)
        seen = {}
        for ev in summary.read_events(path):
            if ev["file_version"] is not None:
                print("file_version %s  wall_time %.3f" % (ev["file_version"], ev["wall_time"]))
            for v in ev["values"]:
                if "simple_value" in v:
                    kind, text = "scalar", "%.9g" % v["simple_value"]
                elif "histo" in v:
                    h = v["histo"]
                    kind = "histogram"
                    text = "num %d  min %.6g  max %.6g  sum %.6g  %d non-empty buckets" % (h["num"], h["min"], h["max"], h["sum"],
                                                                                          sum(1 for c in h["bucket"] if c > 0))
                elif "image" in v:
                    kind, text = "image", "%d x %d, %d bytes of PNG" % (v["image"]["height"], v["image"]["width"], len(v["image"]["png"]))
                else:
                    kind, text = "other", ""
                if args.tags_only:
                    e = seen.setdefault(v.get("tag"), [kind, 0, ev["step"], ev["step"]])
                    e[1], e[3] = e[1] + 1, ev["step"]
                else:
                    print("step %-7d %-9s %-60s %s" % (ev["step"], kind, v.get("tag"), text))
        for tag, (kind, n, s0, s1) in seen.items():
            print("%-9s %-60s %d events, steps %d .. %d" % (kind, tag, n, s0, s1))


if __name__ == "__main__":
    main()
