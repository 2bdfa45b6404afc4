"""dst_nj_bootstrap timing: one JSON line per shape on GPU 0, plain dst_nj and the bootstrap in one
process on the same set.

    python tools/nj_bootstrap_bench.py [--replicates B ...] [--only NAME ...]

Shapes: 2,000 x 30,000 and 10,000 x 30,000 raw on the tools/synth alignment.  Per line: ms per dst_nj call (median of
three after a warm-up call), ms per replicate of one dst_nj_bootstrap call of B replicates (wall time / B, after a
one-replicate warm-up call), and their ratio: the model expects at most 1.10 (resampling, pack and fill in well under a
millisecond beside the rounds).  The resampling kernels' own times: the same script under
`rocprofv3 --kernel-trace --stats`.
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

SHAPES = [   # name, records, sites, measure, replicates
    ("boot2k_raw", 2_000, 30_000, "raw", 20),
    ("boot10k_raw", 10_000, 30_000, "raw", 6),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, nargs="*", default=None, help="one count per shape, in order")
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    with da.Engine(0) as eng:
        for k, (name, n, L, measure, reps) in enumerate(SHAPES):
            if args.only and name not in args.only:
                continue
            if args.replicates:
                reps = args.replicates[min(k, len(args.replicates) - 1)]
            codes = synth.alignment(synth.SEED, n, L)
            eng.upload(0, codes)
            eng.nj(measure)   # warm-up: code objects, slab scratch
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                parent, _ = eng.nj(measure)
                times.append((time.perf_counter() - t0) * 1e3)
            nj_ms = float(np.median(times))
            eng.nj_bootstrap(measure, codes, parent, 1, seed=1)   # warm-up
            t0 = time.perf_counter()
            support = eng.nj_bootstrap(measure, codes, parent, reps, seed=1)
            boot_ms = (time.perf_counter() - t0) * 1e3
            inner = support[n:2 * n - 3]
            print(json.dumps({
                "shape": name, "records": n, "sites": L, "measure": measure, "replicates": reps,
                "nj_ms_per_call": round(nj_ms, 1), "nj_ms_min": round(min(times), 1),
                "bootstrap_ms_total": round(boot_ms, 1), "bootstrap_ms_per_replicate": round(boot_ms / reps, 1),
                "ratio_to_nj": round(boot_ms / reps / nj_ms, 3),
                "splits_with_full_support": int((inner == reps).sum()), "splits_without_support": int((inner == 0).sum()),
                "internal_splits": int(len(inner)), "path": eng.last_path(),
            }), flush=True)


if __name__ == "__main__":
    main()
