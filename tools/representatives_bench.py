"""dst_representatives timing: one JSON line per shape, setting and values on / off on GPU 0, with
dst_clusters at the same threshold on the same upload as the yardstick (the same sweep with an O(n) consumer).

    python tools/representatives_bench.py [--steps 5] [--only NAME ...] [--max-pairs P]

Shapes: 10,000 and 50,000 x 30,000 on the tools/synth alignment.  Settings: `n` at T = 2, and `raw` at the threshold that
links 1e-4 of the pairs (that quantile of the values of every 97th record against the set).  Per line: ms per
dst_representatives call and per dst_clusters call (median, minimum and maximum of --steps calls after one warm-up each;
the two are timed alternately, so both see the same machine), their ratio, the representatives and their share of the
records, dst_clusters' clusters and links, and the launches one call queues behind its pair kernels (sub-blocks x 2, or
x 3 with values).  The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
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
from tools.clusters_bench import slab_count  # noqa: E402

SHAPES = [("r2", 10_000, 30_000), ("r3", 50_000, 30_000)]   # name, records, sites
BLOCK_ROWS = 512   # kRepBlockRows


def raw_threshold(eng, codes, share=1e-4):
    rows = np.arange(0, len(codes), 97)
    eng.upload(1, np.ascontiguousarray(codes[rows]))
    sample = eng.run_rect("raw", 1, 0)
    sample[np.arange(len(rows)), rows] = np.nan
    return float(np.quantile(sample[np.isfinite(sample)], share))


def sub_blocks(n, max_pairs):
    """Sub-blocks of one call: every slab of dst_clusters' cut taken in runs of BLOCK_ROWS rows."""
    bound, blocks, rb = max_pairs or 1 << 25, 0, 0
    while rb < n - 1:
        pairs, re = 0, rb
        while re < n and (re == rb or pairs + (n - re - 1) <= bound):
            pairs += n - re - 1
            re += 1
        blocks += -(-(re - rb) // BLOCK_ROWS) if pairs else 0
        rb = re
    return blocks


def spread(times):
    return {"median": round(float(np.median(times)), 3), "min": round(min(times), 3), "max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--max-pairs", type=int, default=0, help="slab bound (0: the library's default)")
    args = ap.parse_args()
    with da.Engine(0) as eng:
        for name, n, L in SHAPES:
            if args.only and name not in args.only:
                continue
            codes = synth.alignment(synth.SEED, n, L)
            eng.upload(0, codes)
            for measure, t in (("n", 2.0), ("raw", raw_threshold(eng, codes))):
                for values in (False, True):
                    eng.representatives(measure, t, args.max_pairs, values=values)   # warm-up: buffers, lists, schedules
                    eng.clusters(measure, t, args.max_pairs)
                    rep_ms, clu_ms = [], []
                    for _ in range(args.steps):
                        t0 = time.perf_counter()
                        rep = eng.representatives(measure, t, args.max_pairs, values=values)[0]
                        t1 = time.perf_counter()
                        labels, links = eng.clusters(measure, t, args.max_pairs)
                        t2 = time.perf_counter()
                        rep_ms.append((t1 - t0) * 1e3)
                        clu_ms.append((t2 - t1) * 1e3)
                    kept = int(np.count_nonzero(rep == np.arange(n)))
                    blocks = sub_blocks(n, args.max_pairs)
                    print(json.dumps({
                        "shape": name, "records": n, "sites": L, "measure": measure, "threshold": t, "values": values,
                        "max_pairs": args.max_pairs, "steps": args.steps, "representatives_ms": spread(rep_ms),
                        "clusters_ms": spread(clu_ms),
                        "ratio_to_clusters": round(float(np.median(rep_ms) / np.median(clu_ms)), 3),
                        "representatives": kept, "representative_share": round(kept / n, 6),
                        "clusters": int(np.count_nonzero(labels == np.arange(n))), "links": links,
                        "link_share": round(links / (n * (n - 1) / 2), 8),
                        "pair_launches_per_call": slab_count(n, args.max_pairs), "sub_blocks_per_call": blocks,
                        "launches_behind_the_pair_kernels": blocks * (3 if values else 2), "path": eng.last_path(),
                    }), flush=True)


if __name__ == "__main__":
    main()
