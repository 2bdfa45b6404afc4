"""dst_window_group_summary timing: one JSON line per (shape, layout, form, measure) on GPU 0, tools/synth
alignments.

    python tools/window_group_summary_bench.py [--shape scan|square|cells|all] [--measures n,tn93] [--steps 5]
                                               [--out profiles/window_groups/window_group_summary_bench.jsonl] [--no-host]

Shapes, all in the 146 windows of `--windows 1000 --step 200` over 30,000 sites: `scan`, 16 queries (one group) x 10,000
records in 3 and in 64 column groups, each contiguous and interleaved record by record, the cells alone and with the
per-record arrays; `square`, 2,000 records in 3 contiguous groups against themselves, both forms; `cells`, 50,000 records in
3 contiguous groups against themselves, the cells alone.  Per line, in ONE process and alternating between the variants on
every step (one warm-up of each first), the median, the smallest and the largest of --steps:
  groups_ms       (a) one dst_window_group_summary call, its result in host memory, the call's own wait included;
  host_reduce_ms  (b) the same answer the only way there was before: dst_run_windows_host (DST_OUT_DISTANCE) and a numpy
                      reduction by label; its result is compared with (a)'s bitwise in the same run (`same_result`), and
                      `host_run_ms` is the share of the dst_run_windows_host call;
  summary_ms      (c) one dst_window_summary call on the same shape (the totals alone for the cells, with the per-record
                      arrays for the tables): the same sweep with the plain reduction;
and from them the ratios (b) / (a) and (a) / (c).  Neither (b) nor (c) runs the new code.  At `cells` (b) does not exist
(the result would have 1.8e11 entries).  --no-host leaves (b) out.  A library built with measurement flags is refused."""
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
from distance_amd import _lib  # noqa: E402
from tools import synth  # noqa: E402

SCALE_BITS = 37
TOP = np.uint64(1 << 63)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
QUIET_NAN = np.uint64(0x7FF8000000000000)


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def per_pair(vals, threshold):
    """dst_summary's per-pair quantities of DST_OUT_DISTANCE payloads: link, summable, q (0 where not summable), NaN, sort key"""
    if vals.dtype == np.int64:
        return (vals <= np.int64(np.floor(threshold)), np.ones(vals.shape, bool), vals, np.zeros(vals.shape, bool),
                vals.view(np.uint64) ^ TOP)
    with np.errstate(invalid="ignore"):
        ok = np.abs(vals) < 2.0 ** 25
        link = vals <= threshold
    q = np.rint(np.where(ok, vals, 0.0) * 2.0 ** SCALE_BITS).astype(np.int64)
    b = vals.view(np.uint64)
    mag = b & ~TOP
    key = np.where(b >> np.uint64(63) != 0, ~b, b | TOP)
    key = np.where(mag == 0, TOP, key)
    nan = np.isnan(vals)
    return link, ok, q, nan, np.where(nan, ALL_ONES, key)


def payload_of_key(key, int_payload):
    return key ^ TOP if int_payload else np.where(key & TOP != 0, key & ~TOP, ~key)


def to_double(sums, int_payload):
    d = sums.astype(np.float64)   # (int64 to double: round to nearest even, once)
    return d if int_payload else np.ldexp(d, -SCALE_BITS)


def exact_bincount(index, q, size):
    """sums of int64 q per index, exact: two halves whose float64 sums stay below 2^53"""
    lo, hi = q & np.int64(0xFFFFFF), q >> np.int64(24)
    assert int(np.abs(hi).max(initial=0)) * max(len(q), 1) < 2 ** 53
    return (np.bincount(index, hi, size).astype(np.int64) << np.int64(24)) + np.bincount(index, lo, size).astype(np.int64)


class ByLabel:
    """the numpy reduction by label of one window's payloads; the index arrays are built once per shape"""

    def __init__(self, n_rows, n_cols, square, rg, Gr, cg, Gc, per_record):
        if square:
            i, j = np.triu_indices(n_cols, 1)
        else:
            i, j = np.divmod(np.arange(n_rows * n_cols), n_cols)
        self.n_rows, self.square, self.Gr, self.Gc, self.per_record = n_rows, square, Gr, Gc, per_record
        self.cell = rg[i].astype(np.int64) * Gc + cg[j]
        self.order = np.argsort(self.cell, kind="stable")   # for the cells' smallest and largest key
        sorted_cells = self.cell[self.order]
        self.starts = np.flatnonzero(np.r_[True, sorted_cells[1:] != sorted_cells[:-1]])
        self.present = sorted_cells[self.starts]
        if per_record:
            self.rec_i = i.astype(np.int64) * Gc + cg[j]
            self.rec_j = j.astype(np.int64) * Gc + rg[i] if square else None
        row_size, col_size = np.bincount(rg, minlength=Gr).astype(np.int64), np.bincount(cg, minlength=Gc).astype(np.int64)
        self.pairs = np.outer(row_size, col_size)
        if square:
            self.pairs[np.diag_indices(Gr)] = row_size * (row_size - 1) // 2

    def __call__(self, vals, threshold):
        int_payload = vals.dtype == np.int64
        Gr, Gc, cells = self.Gr, self.Gc, self.Gr * self.Gc
        link, ok, q, nan, key = per_pair(vals, threshold)
        grid = lambda x: x.reshape(Gr, Gc)
        n_nan, n_ok, n_link = (grid(np.bincount(self.cell[m], minlength=cells)) for m in (nan, ok, link))
        total = grid(exact_bincount(self.cell, q, cells))
        kmin, kmax = np.full(cells, ALL_ONES), np.zeros(cells, np.uint64)
        real = np.where(nan, np.uint64(0), key)[self.order]
        kmin[self.present] = np.minimum.reduceat(key[self.order], self.starts)
        kmax[self.present] = np.maximum.reduceat(real, self.starts)
        kmin, kmax = grid(kmin), grid(kmax)
        if self.square:
            off = ~np.eye(Gr, dtype=bool)
            n_nan, n_ok, n_link, total = (np.where(off, x + x.T, x) for x in (n_nan, n_ok, n_link, total))
            kmin, kmax = np.where(off, np.minimum(kmin, kmin.T), kmin), np.where(off, np.maximum(kmax, kmax.T), kmax)
        empty = np.uint64(0) if int_payload else QUIET_NAN
        some = self.pairs > n_nan
        out = np.zeros((Gr, Gc, 7), np.uint64)
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = self.pairs, n_nan, n_ok, n_link
        out[..., 4] = to_double(total, int_payload).view(np.uint64)
        out[..., 5] = np.where(some, payload_of_key(kmin, int_payload), empty)
        out[..., 6] = np.where(some, payload_of_key(kmax, int_payload), empty)
        if not self.per_record:
            return out, None, None, None
        size = self.n_rows * Gc
        sides = [self.rec_i] + ([self.rec_j] if self.square else [])
        within = sum(np.bincount(s[link], minlength=size) for s in sides).astype(np.uint32)
        summable = sum(np.bincount(s[ok], minlength=size) for s in sides).astype(np.uint32)
        sums = to_double(sum(exact_bincount(s, q, size) for s in sides), int_payload)
        return out, within, summable, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["scan", "square", "cells", "all"])
    ap.add_argument("--measures", default="n,tn93")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="leave baseline (b) out")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    lib = da.load()
    flags = lib.dst_build_flags().decode()
    if flags:
        raise SystemExit(f"libdistance_hip.so is a measurement build ({flags}): this tool times production builds only")
    L = 30_000
    windows = da.sliding_windows(L, 1000, 200)
    nw = len(windows)
    wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
    # (shape, rows, columns, [(column groups, layout)], [per_record], baseline (b))
    shapes = [("scan", 16, 10_000, [(3, "contiguous"), (3, "interleaved"), (64, "contiguous"), (64, "interleaved")], [False, True], True),
              ("square", 2_000, 2_000, [(3, "contiguous")], [False, True], True),
              ("cells", 50_000, 50_000, [(3, "contiguous")], [False], False)]
    for name, n_rows, n_cols, layouts, forms, has_host in shapes:
        if args.shape not in (name, "all"):
            continue
        square = name != "scan"
        cols = synth.alignment(synth.SEED, n_cols, L)
        rows = cols if square else synth.alignment(synth.SEED ^ 1, n_rows, L)
        P = n_cols * (n_cols - 1) // 2 if square else n_rows * n_cols
        host = has_host and not args.no_host
        with da.Engine(0) as eng:
            eng.upload(0, rows)
            if not square:
                eng.upload(1, cols)
            for (G, layout), per_record, measure in ((x, y, z) for x in layouts for y in forms for z in args.measures.split(",")):
                m = da.MEASURES[measure]
                int_payload = measure in da.INT_MEASURES
                threshold = 30.0 if int_payload else 0.03
                cg = (np.arange(n_cols) * G // n_cols if layout == "contiguous" else np.arange(n_cols) % G).astype(np.uint32)
                rg, Gr = (cg, G) if square else (np.zeros(n_rows, np.uint32), 1)
                n_cells, entries = nw * Gr * G, nw * n_rows * G if per_record else 0
                cells = np.zeros(n_cells * 7, np.uint64)
                within, summable = np.zeros(max(entries, 1), np.uint32), np.zeros(max(entries, 1), np.uint32)
                sums = np.zeros(max(entries, 1), np.float64)
                tot = (_lib.SummaryTotals * nw)()
                s_entries = nw * n_rows if per_record else 0
                s_within, s_summable = np.zeros(max(s_entries, 1), np.uint32), np.zeros(max(s_entries, 1), np.uint32)
                s_sums = np.zeros(max(s_entries, 1), np.float64)
                h_full = np.zeros(nw * P if host else 1, np.int64 if int_payload else np.float64)
                by_label = ByLabel(n_rows, n_cols, square, rg, Gr, cg, G, per_record) if host else None
                host_run, reduced = [], []
                ptr = lambda a: a.ctypes.data if per_record else None

                def groups_call():
                    eng._check(lib.dst_window_group_summary(eng._h, m, int(square), 0, 1, wb.ctypes.data, we.ctypes.data, nw,
                                                            rg.ctypes.data, Gr, cg.ctypes.data, G, threshold, cells.ctypes.data,
                                                            n_cells, ptr(within), ptr(summable), ptr(sums), entries))

                def host_call():
                    t0 = time.perf_counter()
                    eng._check(lib.dst_run_windows_host(eng._h, m, int(square), 0, 1, 0, n_rows, wb.ctypes.data, we.ctypes.data, nw,
                                                        0, h_full.ctypes.data, h_full.nbytes))
                    host_run.append((time.perf_counter() - t0) * 1e3)
                    reduced[:] = [by_label(v, threshold) for v in h_full.reshape(nw, P)]

                def summary_call():
                    eng._check(lib.dst_window_summary(eng._h, m, int(square), 0, 1, wb.ctypes.data, we.ctypes.data, nw, threshold,
                                                      tot, ptr(s_within), ptr(s_summable), ptr(s_sums), s_entries))

                def timed(fn):   # (every call here waits for its own work: synchronous on the context's stream)
                    t0 = time.perf_counter()
                    fn()
                    return (time.perf_counter() - t0) * 1e3

                groups_call()   # warm-up: planes, tables, state
                summary_call()
                if host:
                    host_call()
                host_run.clear()
                a, b, c = [], [], []
                for _ in range(args.steps):   # alternating
                    a.append(timed(groups_call))
                    if host:
                        b.append(timed(host_call))
                    c.append(timed(summary_call))
                got = cells.reshape(nw, Gr, G, 7)
                out = {"shape": name, "rows": n_rows, "cols": n_cols, "sites": L, "square": square, "windows": nw, "pairs": P,
                       "pair_windows": P * nw, "measure": measure, "threshold": threshold, "steps": args.steps, "row_groups": Gr,
                       "col_groups": G, "layout": layout, "per_record": per_record, "groups_ms": stats(a),
                       "full_result_bytes": nw * P * 8, "groups_result_bytes": n_cells * 56 + entries * 16,
                       "links": int(got[..., 3].sum()), "nan_pairs": int(got[..., 1].sum())}
                if host:
                    same = all(np.array_equal(got[w], r[0]) for w, r in enumerate(reduced))
                    if per_record:
                        shape = (nw, n_rows * G)
                        same = same and all(np.array_equal(within.reshape(shape)[w], r[1]) and
                                            np.array_equal(summable.reshape(shape)[w], r[2]) and
                                            np.array_equal(sums.view(np.uint64).reshape(shape)[w], r[3].view(np.uint64))
                                            for w, r in enumerate(reduced))
                    out["same_result"] = bool(same)
                    out["host_reduce_ms"] = stats(b)
                    out["host_run_ms"] = stats(host_run)
                    out["host_reduce_over_groups"] = round(out["host_reduce_ms"]["median"] / out["groups_ms"]["median"], 2)
                out["summary_ms"] = stats(c)
                out["groups_over_summary"] = round(out["groups_ms"]["median"] / out["summary_ms"]["median"], 2)
                line = json.dumps(out)
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")
                if host and not out["same_result"]:
                    raise SystemExit("the host reduction and dst_window_group_summary disagree")


if __name__ == "__main__":
    main()
