"""dst_run_pairs timing: JSON lines on GPU 0 for the tools/synth alignment, lists of random pairs.

    python tools/run_pairs_bench.py [--records 50000] [--sites 30000] [--measures n,tn93] [--sizes 1000,100000,10000000]
                                    [--sorted-sizes 100000] [--steps 5] [--out profiles/run_pairs/run_pairs_bench.jsonl]

Per (measure, list) one line.  What is timed, host clock around calls that return when the result is in host memory, in
--steps rounds that alternate the candidates after one warm-up round each (median, min, max in ms):
  direct      Engine.run_pairs(route="direct"), values
  sweep       Engine.run_pairs(route="sweep"), values
  before      what there was before dst_run_pairs: run_square over the row slabs (2^25 pairs at most) that hold a listed pair,
              into host memory, and a numpy lookup at the canonical positions.  Its result is compared bitwise with both routes
              in the run ("equal").
  count_only  dst_pair_sites(count_only) on the same list: the bandwidth yardstick of the gather (one pass over the four base
              planes of both records)
The lists of --sorted-sizes are also timed sorted by (row, col); their lines carry "host_sort", what a caller pays to get
there from the unsorted list on the host: numpy's lexsort of (row, col), the two index arrays permuted, and a result
scattered back into the list's order (no GPU in it; timed --steps times on the machine the bench runs on).  "lines" is the direct route's model of its traffic, 2 x NP x
nchunks 128-byte lines per pair; "direct_ns_per_line" = direct / (pairs x lines).  The last line of a measure gives the
crossover the figures imply.  Both routes are taken as fixed + per entry x pairs, fitted through the smallest and the
largest unsorted list that touch every slab (the sweep's fixed part is the slabs' pair kernels): the crossover is the list
size at which the two lines meet, null when the sweep's cost per entry is not below the direct route's.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402

SLAB_PAIRS = 1 << 25
PLANES = {"n": 4, "n_high": 4, "raw": 5, "jc69": 5, "k80": 4, "tn93": 3}   # M::NP of the measure's traits


def row_slabs(n):
    """row ranges of the square of at most SLAB_PAIRS pairs each (at least one row)"""
    per_row = n - 1 - np.arange(n - 1, dtype=np.int64)
    bounds, rb = [0], 0
    acc = 0
    for r, p in enumerate(per_row.tolist()):
        if r > rb and acc + p > SLAB_PAIRS:
            bounds.append(r)
            rb, acc = r, 0
        acc += p
    bounds.append(n - 1)
    return np.array(bounds, np.int64)


def before(eng, measure, n, bounds, lo, hi):
    """the values of the canonical pairs (lo, hi) from run_square of the slabs they fall into, looked up on the host"""
    out = None
    slab = np.searchsorted(bounds, lo, side="right") - 1
    for s in np.unique(slab).tolist():
        rb, re = int(bounds[s]), int(bounds[s + 1])
        block = eng.run_square(measure, rb, re)
        if out is None:
            out = np.empty(lo.size, block.dtype)
        sel = slab == s
        i, j = lo[sel], hi[sel]
        first = rb * (2 * n - rb - 1) // 2
        out[sel] = block[i * (2 * n - i - 1) // 2 + (j - i - 1) - first]
    return out


def stats(times):
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50_000)
    ap.add_argument("--sites", type=int, default=30_000)
    ap.add_argument("--measures", default="n,tn93")
    ap.add_argument("--sizes", default="1000,100000,10000000")
    ap.add_argument("--sorted-sizes", default="100000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-before", action="store_true", help="leave the full-run yardstick out")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    n, L = args.records, args.sites
    nchunks = max((L + 127) // 128, 1)
    codes = synth.alignment(synth.SEED, n, L)
    bounds = row_slabs(n)
    rng = np.random.default_rng(12345)
    lists, sort_ms = [], {}
    sorted_sizes = {int(float(x)) for x in args.sorted_sizes.split(",") if x}
    for size in [int(float(x)) for x in args.sizes.split(",")]:
        row, col = rng.integers(0, n, size), rng.integers(0, n, size)
        col = np.where(row == col, (col + 1) % n, col)   # (no diagonal: the full run has none)
        lists.append((size, False, row, col))
        if size in sorted_sizes:
            times = []
            for _ in range(args.steps + 1):   # (the first one is the warm-up)
                t0 = time.perf_counter()
                order = np.lexsort((col, row))
                srow, scol = row[order], col[order]
                back = np.empty(size, np.float64)
                back[order] = srow.astype(np.float64)   # (a result of the sorted list put back in the list's order)
                times.append((time.perf_counter() - t0) * 1e3)
            sort_ms[size] = stats(times[1:])
            lists.append((size, True, srow, scol))

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for measure in args.measures.split(","):
            lines = 2 * PLANES[measure] * nchunks
            fit = []   # (pairs, direct ms, sweep ms) of the unsorted lists that touch every slab
            for size, is_sorted, row, col in lists:
                lo, hi = np.minimum(row, col), np.maximum(row, col)
                results, infos = {}, {}

                def run_direct():
                    results["direct"], infos["direct"] = eng.run_pairs(measure, row, col, route="direct", info=True)

                def run_sweep():
                    results["sweep"], infos["sweep"] = eng.run_pairs(measure, row, col, route="sweep", info=True)

                def run_before():
                    results["before"] = before(eng, measure, n, bounds, lo, hi)

                def run_count():
                    results["count_only"] = eng.pair_sites(measure, row, col, count_only=True)

                what = {"direct": run_direct, "sweep": run_sweep, "count_only": run_count}
                if not args.no_before:
                    what["before"] = run_before
                for fn in what.values():   # warm-up: buffers, planes, lists
                    fn()
                times = {k: [] for k in what}
                for _ in range(args.steps):
                    for k, fn in what.items():
                        t0 = time.perf_counter()
                        fn()
                        times[k].append((time.perf_counter() - t0) * 1e3)
                ref = results.get("before", results["direct"])
                equal = {k: bool(np.array_equal(results[k].view(np.uint64), ref.view(np.uint64))) for k in ("direct", "sweep")}
                auto_info = eng.run_pairs(measure, row, col, route="auto", info=True)[1]
                out = {"records": n, "sites": L, "measure": measure, "pairs": size, "sorted": is_sorted, "steps": args.steps,
                       "lanes_per_pair": infos["direct"]["lanes_per_pair"], "lines_per_pair": lines,
                       "slabs_swept": infos["sweep"]["slabs"], "slabs_of_the_square": int(bounds.size - 1),
                       "auto_route": auto_info["route"], "equal_to_before" if "before" in results else "equal_to_direct": equal}
                for k in what:
                    out[k] = stats(times[k])
                if is_sorted:
                    out["host_sort"] = sort_ms[size]
                d = out["direct"]["median_ms"]
                out["direct_ns_per_pair"] = round(d * 1e6 / size, 2)
                out["direct_ns_per_line"] = round(d * 1e6 / size / lines, 4)
                out["direct_line_GBps"] = round(size * lines * 128 / (d * 1e-3) / 1e9, 1)
                out["count_only_line_GBps"] = round(size * 8 * nchunks * 128 / (out["count_only"]["median_ms"] * 1e-3) / 1e9, 1)
                emit(out)
                if not is_sorted and infos["sweep"]["slabs"] == bounds.size - 1:
                    fit.append((size, out["direct"]["median_ms"], out["sweep"]["median_ms"]))
            if len(fit) >= 2:
                (p0, d0, s0), (p1, d1, s1) = fit[0], fit[-1]
                d_entry, s_entry = (d1 - d0) * 1e6 / (p1 - p0), (s1 - s0) * 1e6 / (p1 - p0)
                d_fixed, s_fixed = d0 * 1e6 - d_entry * p0, s0 * 1e6 - s_entry * p0
                cross = int((s_fixed - d_fixed) / (d_entry - s_entry)) if d_entry > s_entry else None
                emit({"records": n, "sites": L, "measure": measure, "fitted_through_pairs": [p0, p1],
                      "direct_fixed_ms": round(d_fixed * 1e-6, 3), "direct_ns_per_entry": round(d_entry, 2),
                      "sweep_fixed_ms": round(s_fixed * 1e-6, 3), "sweep_ns_per_entry": round(s_entry, 2),
                      "crossover_pairs": cross,
                      "sweep_fixed_ns_per_site_pair": round(s_fixed / (n * (n - 1) / 2) / L, 9)})


if __name__ == "__main__":
    main()
