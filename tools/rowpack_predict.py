"""What packed row tiles can save, priced from a CALD_PROFILE_DUMP launch log (bench.py) of per-view tiling: per layer class the time, the
share of the issued 128-row tile slots that hold no row (1 - true rows / (128 x tiles); true rows from the booked FLOPs), and time x that
share -- the upper bound of the gain if a launch's time were proportional to the rows it issues.  Launches that keep per-view tiles are left
out: the stem (Cin 4), the fused layer-1 pair, gathered rows, the fp16 look-ahead, and the RoI-head GEMMs (rows counted on the device).

    python tools/rowpack_predict.py launches.csv [more.csv ...]
"""
import collections
import csv
import re
import sys

ROI_HEAD = {(12544, 1024), (1024, 1024), (1024, 105), (1024, 455)}      # fc6, fc7, predictor (21 / 91 classes): dyn_rows


def fields(desc):
    d = dict(kv.split("=", 1) for kv in desc.split(",") if "=" in kv)
    kh, kw = (int(x) for x in d["k"].split("x")[:2]) if "+" not in d["k"] else (0, 0)
    return int(d["mt"]), int(d["Cin"]), int(d["Cout"]), kh, kw


def main(path, top=30):
    agg = collections.OrderedDict()
    total_ms = 0.0
    for r in csv.DictReader(open(path)):
        ms = float(r["ms"]); total_ms += ms
        desc = r["desc"]
        mt, cin, cout, kh, kw = fields(desc)
        if "fused" in desc or "gathered" in desc or "lookahead" in desc or "head=" in desc or cin == 4 or (cin, cout) in ROI_HEAD or mt == 0:
            continue
        rows = float(r["gflop"]) * 1e9 / (2.0 * cout * kh * kw * cin)
        a = agg.setdefault(re.sub(r"mt=\d+,", "", desc), [0, 0.0, 0.0, 0.0, 0.0])
        a[0] += 1; a[1] += ms; a[2] += rows; a[3] += 128.0 * mt; a[4] += ms * (1.0 - rows / (128.0 * mt))
    save = sum(a[4] for a in agg.values())
    print("%s: %.1f ms of conv / linear launches, %.1f ms in packable classes, predicted saving %.2f ms = %.2f%% of the launch time" % (
        path, total_ms, sum(a[1] for a in agg.values()), save, 100.0 * save / total_ms))
    for k, a in sorted(agg.items(), key=lambda kv: -kv[1][4])[:top]:
        print("  %-40s n=%5d %9.2f ms  empty slots %5.2f%%  saving %7.3f ms" % (k[:40], a[0], a[1], 100.0 * (1.0 - a[2] / a[3]), a[4]))


if __name__ == "__main__":
    for p in sys.argv[1:]:
        main(p)
