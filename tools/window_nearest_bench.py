"""dst_nearest_windows timing: one JSON line per (shape, measure, K) on GPU 0, tools/synth alignments.

    python tools/window_nearest_bench.py [--shape scan|square|both] [--measures n,tn93] [--steps 5]
                                         [--out profiles/window_nearest/window_nearest_bench.jsonl] [--kernel-only]

Shapes: `scan`, 16 queries x 10,000 records x 30,000 sites with the windows of `--windows 1000 --step 200` (146 of them), a
rectangle, K = 1 and 10; `square`, 2,000 records x 30,000 sites against themselves in the same 146 windows, K = 5.  Per
line, in ONE process and alternating between the variants on every step (one warm-up of each first), the median, the
smallest and the largest of --steps:
  nearest_ms      (a) one dst_nearest_windows call: index and values in host memory, the call's own wait included;
  host_select_ms  (b) the same answer the way it was had without it: dst_run_windows_host (DST_OUT_DISTANCE) and a numpy
                      selection of the k smallest (key, record) per (row, window); its index is compared with (a)'s
                      bitwise in the same run (`same_index`), and `host_run_ms` is the share of the dst_run_windows_host call;
  sweep_ms        (c) one dst_run_windows call into device memory, DST_OUT_DISTANCE: the sweep alone, the floor (a square
                      sweeps the triangle there and the whole square in (a): half the work);
and from them the ratios (b) / (a) and (a) / (c).  Neither (b) nor (c) runs the new code.  --kernel-only: only the
dst_nearest_windows calls, for a profiler's run."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import distance_amd as da  # noqa: E402
from distance_amd import _lib  # noqa: E402
from tools import synth  # noqa: E402

TOP = np.uint64(0xFFFFFFFFFFFFFFFF)


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def keys(vals):
    """dst_nearest's sort key of DST_OUT_DISTANCE payloads"""
    if vals.dtype == np.int64:
        return vals.view(np.uint64) ^ np.uint64(1 << 63)
    b = vals.view(np.uint64)
    k = np.where((b >> np.uint64(63)) == 1, ~b, b | np.uint64(1 << 63))
    k[vals == 0] = np.uint64(1 << 63)
    k[np.isnan(vals)] = TOP
    return k


def select(key, k, own=None):
    """the k smallest (key, column) of every row of key[rows, cols], in that order; own[r]: a column of row r left out.
    A partition finds every row's (k + 1)-th key, the few entries at or below it are sorted."""
    rows, cols = key.shape
    extra = 0 if own is None else 1
    kth = np.partition(key, k - 1 + extra, axis=1)[:, k - 1 + extra]
    r, c = np.nonzero(key <= kth[:, None])
    if own is not None:
        keep = c != own[r]
        r, c = r[keep], c[keep]
    order = np.lexsort((c, key[r, c], r))
    r, c = r[order], c[order]
    start = np.searchsorted(r, np.arange(rows))
    pos = np.arange(len(r)) - start[r]
    return c[pos < k].reshape(rows, k).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["scan", "square", "both"])
    ap.add_argument("--measures", default="n,tn93")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="only the dst_nearest_windows calls (for a profiler's run)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    lib = da.load()
    L = 30_000
    windows = da.sliding_windows(L, 1000, 200)
    shapes = []
    if args.shape in ("scan", "both"):
        shapes.append(("scan", 16, 10_000, (1, 10)))
    if args.shape in ("square", "both"):
        shapes.append(("square", 2_000, 2_000, (5,)))
    nw = len(windows)
    wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
    for name, n_rows, n_cols, ks in shapes:
        square = name == "square"
        cols = synth.alignment(synth.SEED, n_cols, L)
        rows = cols if square else synth.alignment(synth.SEED ^ 1, n_rows, L)
        P = n_cols * (n_cols - 1) // 2 if square else n_rows * n_cols
        iu = np.triu_indices(n_cols, 1) if square else None
        own = np.arange(n_rows) if square else None
        with da.Engine(0) as eng:
            if square:
                eng.upload(0, cols)
            else:
                eng.upload(0, rows)
                eng.upload(1, cols)
            for measure in args.measures.split(","):
                m = da.MEASURES[measure]
                dtype = np.int64 if measure in da.INT_MEASURES else np.float64
                h_full = np.zeros(nw * P, dtype)
                d_out = torch.zeros(nw * P, dtype=torch.float64, device="cuda")
                for k in ks:
                    index = np.zeros((n_rows, nw, k), np.uint32)
                    values = np.zeros((n_rows, nw, k), dtype)
                    k_used = np.zeros(1, np.uint32)
                    host_index = np.zeros((n_rows, nw, k), np.uint32)
                    host_run = []

                    def nearest_call():
                        eng._check(lib.dst_nearest_windows(eng._h, m, int(square), 0, 1, 0, n_rows, wb.ctypes.data, we.ctypes.data,
                                                           nw, k, 0, index.ctypes.data, None, values.ctypes.data, index.size,
                                                           k_used.ctypes.data_as(_lib._u32p)))

                    def host_select():
                        t0 = time.perf_counter()
                        eng._check(lib.dst_run_windows_host(eng._h, m, int(square), 0, 1, 0, n_rows, wb.ctypes.data, we.ctypes.data,
                                                            nw, 0, h_full.ctypes.data, h_full.nbytes))
                        host_run.append((time.perf_counter() - t0) * 1e3)
                        res = h_full.reshape(nw, P)
                        if not square:
                            got = select(keys(res).reshape(nw * n_rows, n_cols), k)
                            host_index[:] = got.reshape(nw, n_rows, k).transpose(1, 0, 2)
                            return
                        full = np.empty((n_cols, n_cols), np.uint64)
                        for w in range(nw):
                            kw = keys(res[w])
                            full[iu] = kw
                            full[(iu[1], iu[0])] = kw
                            full[own, own] = TOP
                            host_index[:, w] = select(full, k, own)

                    def sweep_call():
                        eng._check(lib.dst_run_windows(eng._h, m, int(square), 0, 1, 0, n_rows, wb.ctypes.data, we.ctypes.data, nw, 0,
                                                       d_out.data_ptr(), d_out.numel() * 8, None))

                    def timed(fn):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        return (time.perf_counter() - t0) * 1e3

                    nearest_call()   # warm-up: planes, tables, scratch
                    if args.kernel_only:
                        for _ in range(args.steps):
                            nearest_call()
                        continue
                    host_select()
                    sweep_call()
                    host_run.clear()
                    a, b, c = [], [], []
                    for _ in range(args.steps):   # alternating
                        a.append(timed(nearest_call))
                        b.append(timed(host_select))
                        c.append(timed(sweep_call))
                    same = bool(int(k_used[0]) == k and np.array_equal(index, host_index))
                    a_s, b_s, c_s = stats(a), stats(b), stats(c)
                    line = json.dumps({
                        "shape": name, "rows": n_rows, "cols": n_cols, "sites": L, "square": square, "windows": nw,
                        "pair_windows": (n_rows * n_cols if square else P) * nw, "measure": measure, "k": k, "steps": args.steps,
                        "same_index": same, "nearest_ms": a_s, "host_select_ms": b_s, "host_run_ms": stats(host_run),
                        "sweep_ms": c_s, "full_result_bytes": nw * P * 8, "nearest_result_bytes": index.nbytes + values.nbytes,
                        "host_select_over_nearest": round(b_s["median"] / a_s["median"], 2),
                        "nearest_over_sweep": round(a_s["median"] / c_s["median"], 2),
                    })
                    print(line, flush=True)
                    if args.out:
                        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                        with open(args.out, "a") as fh:
                            fh.write(line + "\n")


if __name__ == "__main__":
    main()
