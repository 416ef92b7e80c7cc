"""python tools/envelope_profile.py <rows.jsonl> [<ab.jsonl>] > profiles/envelope_corners.json

rows.jsonl: what tests/test_gpu_envelope.py appends with LMPC_ENVELOPE_PROFILE=<rows.jsonl> (one object per case and route).  ab.jsonl (optional): lines
{"which": "parent" | "this", "value": <headline of bench.py --gpus 1 --steps 200 --warmup 20>} of the parent's build and this one, run alternately."""
import json
import statistics
import sys


def main(argv):
    rows = [json.loads(l) for l in open(argv[1]) if l.strip()]
    doc = dict(what="tests/test_gpu_envelope.py::test_every_route_of_every_corner on an MI355X: per case (N, numSS_it, points per lap) and route the batch, waves per QP, dynamic "
                    "LDS per QP in bytes as lmpc_solver_lds reports it (0: no such kernel for the pair), iterations over the 64 problems P, worst errors against the oracle on the "
                    "compared problems (abc, xu, zt relative as common.compare_with_oracle scales them), problems left out of the (x, u) comparison, and the distance of (x, u) "
                    "and zt from the case's first route",
               tolerances=dict(TOL_ABC=1e-9, TOL_XU=1e-6, TOL_ZT=1e-6, TOL_ROUTE=2e-7), rows=rows)
    if len(argv) > 2:
        ab = [json.loads(l) for l in open(argv[2]) if l.strip()]
        p = [r["value"] for r in ab if r["which"] == "parent"]; t = [r["value"] for r in ab if r["which"] == "this"]
        doc["bench_against_parent"] = dict(what="python bench.py --gpus 1 --steps 200 --warmup 20: the parent's build and this one alternating, every run a process of its own",
                                           parent_runs=p, this_runs=t, parent_median=statistics.median(p), parent_range=[min(p), max(p)], this_median=statistics.median(t),
                                           this_median_inside_parent_range=min(p) <= statistics.median(t) <= max(p))
    json.dump(doc, sys.stdout, indent=1)


if __name__ == "__main__":
    main(sys.argv)
