"""Summary of an alternating same-box A/B of bench.py runs: reads DIR/parent_<i>.json and DIR/this_<i>.json (one bench.py result each) and
prints the record kept under profiles/ -- per run the headline figures and the identity fields, then the verdict against the parent's own
spread: the gain counts if every new run beats every parent run and the difference of the means is at least twice the parent's range.

    python tools/ab_summary.py DIR "what was run" > profiles/<name>_ab.json
"""
import glob
import json
import os
import sys


def record(path):
    d = json.load(open(path))
    r = d["roofline"]
    return {
        "value": d["value"], "ms_per_step": d["ms_per_step"], "gemm_ms_per_step": r["gemm_ms_per_step"], "roofline_frac": r["frac"],
        "launches": r["launches"], "algorithmic_gflop_per_launch": r["algorithmic_gflop_per_launch"],
        "lookahead_ms_per_step": r["rpn_prune"]["lookahead_ms_per_step"],
        "selected_sha1": d["config"]["selected_sha1"],
        "pixels_recomputed_exactly": r["rpn_prune"]["pixels_recomputed_exactly"],
        "worst_observed_error_over_bound": r["rpn_prune"]["worst_observed_error_over_bound"],
        "roi_rows_per_view_measured": r["roi_rows_per_view_measured"],
    }


def main(d, what):
    runs = {}
    for side in ("parent", "this"):
        for p in sorted(glob.glob(os.path.join(d, side + "_*.json"))):
            runs[os.path.basename(p)[:-5]] = record(p)
    pv = [r["value"] for k, r in runs.items() if k.startswith("parent")]
    tv = [r["value"] for k, r in runs.items() if k.startswith("this")]
    pm, tm, spread = sum(pv) / len(pv), sum(tv) / len(tv), max(pv) - min(pv)
    ident = {k: len({json.dumps(r[k], sort_keys=True) for r in runs.values()}) == 1
             for k in ("selected_sha1", "pixels_recomputed_exactly", "worst_observed_error_over_bound", "roi_rows_per_view_measured", "launches",
                       "algorithmic_gflop_per_launch")}
    out = {
        "what": what, "runs": runs, "parent_mean": pm, "this_mean": tm, "parent_spread_max_minus_min": spread,
        "this_minus_parent": tm - pm, "this_over_parent": tm / pm,
        "gemm_ms_per_step_parent_mean": sum(r["gemm_ms_per_step"] for k, r in runs.items() if k.startswith("parent")) / len(pv),
        "gemm_ms_per_step_this_mean": sum(r["gemm_ms_per_step"] for k, r in runs.items() if k.startswith("this")) / len(tv),
        "every_new_run_beats_every_parent_run": min(tv) > max(pv),
        "difference_at_least_twice_parent_spread": tm - pm >= 2.0 * spread,
        "identity": ident,
    }
    out["gain_counts"] = out["every_new_run_beats_every_parent_run"] and out["difference_at_least_twice_parent_spread"]
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
