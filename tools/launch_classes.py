"""Per-layer-class summary of a CALD_PROFILE_DUMP launch log (bench.py): time, share and TFLOP/s per (Cin, Cout, filter, stride, group).
With --csv the classes come out as a table (class, launches, tiles, gflop, ms, tflops) small enough to keep under profiles/."""
import collections
import csv
import re
import sys


def classes(path):
    agg = collections.OrderedDict()
    for r in csv.DictReader(open(path)):
        k = re.sub(r"mt=\d+,", "", r["desc"])
        mt = re.search(r"mt=(\d+)", r["desc"])
        a = agg.setdefault(k, [0, 0.0, 0.0, 0])
        a[0] += 1; a[1] += float(r["ms"]); a[2] += float(r["gflop"]); a[3] += int(mt.group(1)) if mt else 0
    return sorted(agg.items(), key=lambda kv: -kv[1][1])


def main(path, top=40):
    agg = classes(path)
    tot = sum(a[1] for _, a in agg); fl = sum(a[2] for _, a in agg)
    print("%s: %d launches, %.1f ms, %.1f TFLOP/s overall" % (path, sum(a[0] for _, a in agg), tot, fl / tot))
    for k, a in agg[:top]:
        print("  %-46s n=%5d %9.2f ms %5.1f%%  %7.1f TF" % (k[:46], a[0], a[1], 100 * a[1] / tot, a[2] / a[1]))


def table(path):
    w = csv.writer(sys.stdout, lineterminator="\n")
    w.writerow(["class", "launches", "tiles", "gflop", "ms", "tflops"])
    for k, a in classes(path):
        w.writerow([k, a[0], a[3], "%.3f" % a[2], "%.4f" % a[1], "%.2f" % (a[2] / a[1])])


if __name__ == "__main__":
    if sys.argv[1:2] == ["--csv"]:
        table(sys.argv[2])
    else:
        for p in sys.argv[1:]:
            main(p)
