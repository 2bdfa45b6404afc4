"""dst_site_counts timing: one JSON line per (size, group layout) on GPU 0, tools/synth alignments.

    python tools/site_counts_bench.py [--sizes 10000,50000] [--sites 30000] [--steps 5]
                                      [--out profiles/site_counts/site_counts_bench.jsonl] [--no-host]

Group layouts: 1 group (no labels); 3 groups contiguous; 3 groups interleaved record by record; 256 interleaved.  Per line,
in ONE process and alternating between the two on every step (one warm-up of each first), the median, the smallest and the
largest of --steps:
  call_ms   (a) one dst_site_counts call over all sites, its result in host memory, the call's own wait included;
  host_ms   (b) the same counts the only way there was before: numpy on the code matrix in host memory (classes from the
                high nibble, summed per group over blocks of columns); compared with (a)'s bitwise in the same run
                (`same_result`);
and beside them floor_ms, the time the four base planes (4 x n x sites / 8 bytes) take at the fill rate bench.py works
with (HBM_FILL_GBS, a write-only rate measured on this kind of box: a floor computed from bytes, not a result), and the
ratios call / floor and host / call.  --no-host leaves (b) out.  A library built with measurement flags is refused."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402
import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402

NIBBLE_CLASS = np.full(16, 255, np.uint8)
NIBBLE_CLASS[[0b1000, 0b0001, 0b0100, 0b0010]] = [0, 1, 2, 3]
for nib in range(1, 15):
    if bin(nib).count("1") >= 2:
        NIBBLE_CLASS[nib] = 4
COLUMN_BLOCK = 512


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def layouts(n):
    r = np.arange(n)
    return {"1 group": (None, 1), "3 contiguous": (np.minimum(r * 3 // n, 2), 3), "3 interleaved": (r % 3, 3),
            "256 interleaved": (r % 256, 256)}


def host_counts(codes, groups, n_groups):
    """(sites, G, 5) uint32 by numpy from the code matrix"""
    n, length = codes.shape
    out = np.zeros((length, n_groups, 5), np.uint32)
    if groups is None:
        order, starts = None, np.zeros(1, np.int64)
    else:
        order = np.argsort(groups, kind="stable")
        starts = np.searchsorted(groups[order], np.arange(n_groups))
    for b in range(0, length, COLUMN_BLOCK):
        cls = NIBBLE_CLASS[codes[:, b:b + COLUMN_BLOCK] >> 4]
        if order is not None:
            cls = cls[order]
        for k in range(5):
            hot = (cls == k).view(np.uint8)
            out[b:b + COLUMN_BLOCK, :, k] = np.add.reduceat(hot, starts, axis=0, dtype=np.uint32).T
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000")
    ap.add_argument("--sites", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    flags = da.load().dst_build_flags().decode()
    if flags:
        raise SystemExit(f"libdistance_hip.so was built with measurement flags ({flags}): not a timing build")
    lines = []
    with da.Engine(0) as eng:
        for n in [int(x) for x in args.sizes.split(",")]:
            codes = synth.alignment(synth.SEED, n, args.sites)
            eng.set_path("dense")   # (every plane stored by the upload: the call is timed without ensure_planes' one-off work)
            eng.upload(0, codes)
            floor_ms = 4 * n * args.sites / 8 / (bench.HBM_FILL_GBS * 1e9) * 1e3
            for name, (groups, G) in layouts(n).items():
                got = eng.site_counts(0, groups, G)   # warm-up of (a)
                same = None
                if not args.no_host:
                    same = bool(np.array_equal(got, host_counts(codes, groups, G)))   # warm-up of (b), and the check
                call, host = [], []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    eng.site_counts(0, groups, G)
                    call.append((time.perf_counter() - t0) * 1e3)
                    if not args.no_host:
                        t0 = time.perf_counter()
                        host_counts(codes, groups, G)
                        host.append((time.perf_counter() - t0) * 1e3)
                line = {"n": n, "sites": args.sites, "layout": name, "groups": G, "entries": int(got.size), "call_ms": stats(call),
                        "floor_ms": round(floor_ms, 4), "call_over_floor": round(float(np.median(call)) / floor_ms, 1),
                        "fill_rate_gbs": bench.HBM_FILL_GBS}
                if host:
                    line.update(host_ms=stats(host), host_over_call=round(float(np.median(host) / np.median(call)), 1),
                                same_result=same)
                print(json.dumps(line), flush=True)
                lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)), exist_ok=True)
        with open(os.path.join(ROOT, args.out), "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
