"""dst_text_matrix timing: one JSON line per shape on GPU 0.

    python tools/matrix_bench.py [--steps 2] [--only NAME ...] [--slab-cells C] [--cli-dir DIR]

Shapes: 50,000 x 30,000 raw and tn93, and 10,000 x 30,000 raw, on the tools/synth alignment.  Per shape: ms per full
matrix (every row, in calls of whole rows of at most --slab-cells cells, into one page-locked buffer; median of --steps
passes after a warm-up pass), GB of text, the pair kernels' share from dst_kernel_ms_mean (mean per launch x calls) and
the rest (the two text kernels, the scan, the copy of the text, host work) as the difference.  The text kernels' own
times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
--cli-dir DIR: also write the shape's FASTA there and time the CLI end to end (`DISTANCE_TIMING=1`, output to /dev/null),
`--matrix tsv` next to the long output of the same input, in the same process tree.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402

SHAPES = [   # name, records, sites, measure
    ("c3_raw", 50_000, 30_000, "raw"),
    ("c3_tn93", 50_000, 30_000, "tn93"),
    ("c2_raw", 10_000, 30_000, "raw"),
]
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


def one_pass(eng, lib, m, n, rows_per_call, buf, cap):
    total, calls = 0, 0
    out = C.c_size_t(0)
    for rb in range(0, n, rows_per_call):
        re = min(n, rb + rows_per_call)
        rc = lib.dst_text_matrix(eng._h, m, 1, 0, 0, rb, re, 0, buf, cap, C.byref(out))
        if rc:
            raise da.DistanceError(rc, lib.dst_last_error(eng._h).decode())
        total += out.value
        calls += 1
    return total, calls


def cli_run(args, env):
    t0 = time.perf_counter()
    r = subprocess.run([CLI] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env, timeout=600)
    ms = (time.perf_counter() - t0) * 1e3
    if r.returncode:
        raise RuntimeError(r.stderr.decode())
    phases = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("[timing]")]
    return ms, phases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--slab-cells", type=int, default=1 << 22, help="cells per call (the CLI's default --slab-pairs)")
    ap.add_argument("--cli-dir", default=None)
    args = ap.parse_args()
    lib = da.load()
    with da.Engine(0) as eng:
        for name, n, L, measure in SHAPES:
            if args.only and name not in args.only:
                continue
            codes = synth.alignment(synth.SEED, n, L)
            ids = ["s%d" % k for k in range(n)]
            eng.upload(0, codes)
            eng.set_ids(0, ids)
            m = da.MEASURES[measure]
            rows_per_call = max(1, args.slab_cells // n)
            cap = rows_per_call * (n * 33 + 64) + 4096
            ptr = C.c_void_p()
            if lib.dst_host_alloc(cap, C.byref(ptr)):
                raise RuntimeError("dst_host_alloc")
            try:
                one_pass(eng, lib, m, n, rows_per_call, ptr, cap)   # warm-up: buffers, lists, schedules
                times, pair_totals = [], []
                for _ in range(args.steps):
                    eng.kernel_ms_mean(reset=True)
                    t0 = time.perf_counter()
                    text_bytes, calls = one_pass(eng, lib, m, n, rows_per_call, ptr, cap)
                    times.append((time.perf_counter() - t0) * 1e3)
                    km = eng.kernel_ms_mean(reset=True)   # mean over the last (up to 64) pair launches
                    pair_totals.append(km["pair_ms"] * calls)
            finally:
                lib.dst_host_free(ptr)
            ms, pair_ms = float(np.median(times)), float(np.median(pair_totals))
            line = {
                "shape": name, "records": n, "sites": L, "measure": measure, "steps": args.steps,
                "cells": n * n, "rows_per_call": rows_per_call, "calls": calls, "ms_per_matrix": round(ms, 1),
                "ms_min": round(min(times), 1), "text_gb": round(text_bytes / 1e9, 3),
                "text_gb_per_s": round(text_bytes / 1e6 / ms, 2), "pair_kernels_ms": round(pair_ms, 1),
                "text_and_copy_ms": round(ms - pair_ms, 1), "path": eng.last_path(),
            }
            if args.cli_dir:
                fa = os.path.join(args.cli_dir, name + ".fasta")
                if not os.path.exists(fa):
                    with open(fa, "wb") as fh:
                        fh.write(synth.fasta_bytes(synth.SEED, codes))
                env = dict(os.environ, DISTANCE_TIMING="1")
                for label, extra in (("long", []), ("matrix_tsv", ["--matrix", "tsv"]), ("long_again", []),
                                     ("matrix_tsv_again", ["--matrix", "tsv"])):
                    cms, phases = cli_run(["-m", measure, "-o", "/dev/null", fa] + extra, env)
                    line["cli_" + label + "_ms"] = round(cms, 1)
                    line["cli_" + label + "_phases"] = phases
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
