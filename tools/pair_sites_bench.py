"""dst_pair_sites timing: one JSON line on GPU 0 for the tools/synth alignment at 10,000 x 30,000, -m n.

    python tools/pair_sites_bench.py [--steps 3] [--records 10000] [--sites 30000] [--out profiles/pair_sites/pair_sites_bench.jsonl]

The yardstick is dst_links at T = 5 handing row, col and tallies to a sink (what `--max-distance 5` runs without --sites);
beside it, in the same session, dst_pair_sites over those links: the count-only call (one pass over the planes) and the
call that returns sites and bases (a count pass and a write pass).  Per line: ms per call (median of --steps calls after
one warm-up), the ratio, and the bytes of planes a pass reads per second: 128 bytes per (pair, 128-site chunk), the 16
bytes of four base planes of two records, counted once per pass whatever the caches served.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402


def timed(fn, steps):
    fn()   # warm-up: buffers, planes
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--records", type=int, default=10_000)
    ap.add_argument("--sites", type=int, default=30_000)
    ap.add_argument("--threshold", type=float, default=5.0)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    args = ap.parse_args()
    lib = da.load()
    n, L = args.records, args.sites
    codes = synth.alignment(synth.SEED, n, L)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        links_ms, links_min, (row, col, tal) = timed(lambda: eng.links("n", args.threshold, values=False, tallies=True), args.steps)
        m = da.MEASURES["n"]
        pairs = int(row.size)
        offsets = np.zeros(pairs + 1, np.uint64)
        total = C.c_uint64()
        cap = max(int(tal[:, 0].sum()), 1)   # (the difference tally sizes the buffers, as the CLI does it)
        sites, bases = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)

        def count():
            eng._check(lib.dst_pair_sites(eng._h, m, 1, 0, 1, row.ctypes.data, col.ctypes.data, pairs, offsets.ctypes.data, None,
                                          None, 0, C.byref(total)))
            return int(total.value)

        def full():
            eng._check(lib.dst_pair_sites(eng._h, m, 1, 0, 1, row.ctypes.data, col.ctypes.data, pairs, offsets.ctypes.data,
                                          sites.ctypes.data, bases.ctypes.data, cap, C.byref(total)))
            return int(total.value)

        if pairs == 0:
            raise SystemExit("no links at this threshold: nothing to time")
        count_ms, count_min, entries = timed(count, args.steps)
        full_ms, full_min, entries2 = timed(full, args.steps)
        assert entries == entries2 == int(tal[:, 0].sum())
        pass_bytes = pairs * ((L + 127) // 128) * 128
        line = json.dumps({
            "records": n, "sites": L, "measure": "n", "threshold": args.threshold, "steps": args.steps, "links": pairs,
            "entries": entries, "links_tallies_ms": round(links_ms, 3), "links_tallies_ms_min": round(links_min, 3),
            "pair_sites_count_ms": round(count_ms, 3), "pair_sites_count_ms_min": round(count_min, 3),
            "pair_sites_full_ms": round(full_ms, 3), "pair_sites_full_ms_min": round(full_min, 3),
            "full_over_links": round(full_ms / links_ms, 3), "plane_bytes_per_pass": pass_bytes,
            "count_pass_GBps": round(pass_bytes / (count_ms * 1e-3) / 1e9, 2),
            "full_two_pass_GBps": round(2 * pass_bytes / (full_ms * 1e-3) / 1e9, 2),
        })
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
