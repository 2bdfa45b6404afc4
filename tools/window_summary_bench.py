"""dst_window_summary timing: one JSON line per (shape, measure) on GPU 0, tools/synth alignments.

    python tools/window_summary_bench.py [--shape scan|square|totals|all] [--measures n,tn93] [--steps 5]
                                         [--out profiles/window_summary/window_summary_bench.jsonl] [--kernel-only]

Shapes, all in the 146 windows of `--windows 1000 --step 200` over 30,000 sites: `scan`, 16 queries x 10,000 records, a
rectangle; `square`, 2,000 records against themselves; `totals`, 50,000 records against themselves, the totals only (no
per-record array: O(n_windows) of device state).  Per line, in ONE process and alternating between the variants on every
step (one warm-up of each first), the median, the smallest and the largest of --steps:
  summary_ms      (a) one dst_window_summary call: totals and the three per-record arrays in host memory (`totals`: the
                      totals alone), the call's own wait included;
  host_reduce_ms  (b) the same answer the only way there was before: dst_run_windows_host (DST_OUT_DISTANCE) and a numpy
                      reduction by dst_summary's definition; its result is compared with (a)'s bitwise in the same run
                      (`same_result`), and `host_run_ms` is the share of the dst_run_windows_host call;
  sweep_ms        (c) one dst_run_windows call into device memory, DST_OUT_DISTANCE: the sweep alone, what a fused
                      reduction that writes nothing is held against;
and from them the ratios (b) / (a) and (a) / (c).  Neither (b) nor (c) runs the new code.  At `totals` neither exists (the
result would have 1.8e11 entries): the call's time alone.  `full_square` records whether DST_WINDOW_SUMMARY_FULL_SQUARE was
set: the square's measured alternative, the full square swept with the row side only.  --no-host leaves (b) out, for
the alternative's run.  --kernel-only: only the dst_window_summary calls, for a profiler's run."""
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

SCALE_BITS = 37


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def per_pair(measure, vals, threshold):
    """dst_summary's per-pair quantities of DST_OUT_DISTANCE payloads: link, summable, q (0 where not summable), NaN"""
    if vals.dtype == np.int64:
        return vals <= np.int64(np.floor(threshold)), np.ones(vals.shape, bool), vals, np.zeros(vals.shape, bool)
    with np.errstate(invalid="ignore"):
        ok = np.abs(vals) < 2.0 ** 25
        link = vals <= threshold
    q = np.rint(np.where(ok, vals, 0.0) * 2.0 ** SCALE_BITS).astype(np.int64)
    return link, ok, q, np.isnan(vals)


def to_double(sums, int_payload):
    d = sums.astype(np.float64)   # (int64 to double: round to nearest even, once)
    return d if int_payload else np.ldexp(d, -SCALE_BITS)


def host_reduce(measure, res, n_rows, n_cols, square, threshold, iu):
    """totals[nw, 4] (NaN, summable, links as uint64 and the sum as double bits) and within / summable / sum [nw, n_rows]"""
    nw = res.shape[0]
    int_payload = res.dtype == np.int64
    within = np.zeros((nw, n_rows), np.uint32)
    summable = np.zeros((nw, n_rows), np.uint32)
    sums = np.zeros((nw, n_rows), np.float64)
    tot = np.zeros((nw, 3), np.uint64)
    tsum = np.zeros(nw, np.float64)
    full = np.zeros((n_cols, n_cols), np.int64) if square else None
    for w in range(nw):
        link, ok, q, nan = per_pair(measure, res[w], threshold)
        assert int(np.abs(q).max(initial=0)) * max(n_cols, 1) < 2 ** 62   # no int64 sum below can overflow
        tot[w] = (nan.sum(), ok.sum(), link.sum())
        tsum[w] = to_double(q.sum(dtype=np.int64, keepdims=True), int_payload)[0]
        if square:   # a pair counts for both of its records
            within[w] = np.bincount(iu[0][link], minlength=n_rows) + np.bincount(iu[1][link], minlength=n_rows)
            summable[w] = np.bincount(iu[0][ok], minlength=n_rows) + np.bincount(iu[1][ok], minlength=n_rows)
            full[iu] = q   # (int64 sums: exact)
            sums[w] = to_double(full.sum(axis=1) + full.sum(axis=0), int_payload)
        else:
            within[w] = link.reshape(n_rows, n_cols).sum(axis=1)
            summable[w] = ok.reshape(n_rows, n_cols).sum(axis=1)
            sums[w] = to_double(q.reshape(n_rows, n_cols).sum(axis=1, dtype=np.int64), int_payload)
    return tot, tsum, within, summable, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["scan", "square", "totals", "all"])
    ap.add_argument("--measures", default="n,tn93")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="only the dst_window_summary calls (for a profiler's run)")
    ap.add_argument("--no-host", action="store_true", help="leave baseline (b) out (the alternative's run: (a) and (c) only)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    lib = da.load()
    L = 30_000
    windows = da.sliding_windows(L, 1000, 200)
    nw = len(windows)
    wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
    shapes = [s for s in (("scan", 16, 10_000), ("square", 2_000, 2_000), ("totals", 50_000, 50_000))
              if args.shape in (s[0], "all")]
    for name, n_rows, n_cols in shapes:
        square = name != "scan"
        totals_only = name == "totals"
        cols = synth.alignment(synth.SEED, n_cols, L)
        rows = cols if square else synth.alignment(synth.SEED ^ 1, n_rows, L)
        P = n_cols * (n_cols - 1) // 2 if square else n_rows * n_cols
        iu = np.triu_indices(n_cols, 1) if square and not totals_only else None
        with da.Engine(0) as eng:
            eng.upload(0, rows)
            if not square:
                eng.upload(1, cols)
            for measure in args.measures.split(","):
                m = da.MEASURES[measure]
                int_payload = measure in da.INT_MEASURES
                threshold = 30.0 if int_payload else 0.03
                baselines = not totals_only and not args.kernel_only
                host = baselines and not args.no_host
                tot = (_lib.SummaryTotals * nw)()
                entries = 0 if totals_only else nw * n_rows
                within = np.zeros(max(entries, 1), np.uint32)
                summable = np.zeros(max(entries, 1), np.uint32)
                sums = np.zeros(max(entries, 1), np.float64)
                h_full = np.zeros(nw * P if host else 1, np.int64 if int_payload else np.float64)
                d_out = torch.zeros(nw * P if baselines else 1, dtype=torch.float64, device="cuda")
                host_run, reduced = [], []

                def summary_call():
                    eng._check(lib.dst_window_summary(eng._h, m, int(square), 0, 1, wb.ctypes.data, we.ctypes.data, nw, threshold,
                                                      tot, None if totals_only else within.ctypes.data,
                                                      None if totals_only else summable.ctypes.data,
                                                      None if totals_only else sums.ctypes.data, entries))

                def host_call():
                    t0 = time.perf_counter()
                    eng._check(lib.dst_run_windows_host(eng._h, m, int(square), 0, 1, 0, n_rows, wb.ctypes.data, we.ctypes.data, nw,
                                                        0, h_full.ctypes.data, h_full.nbytes))
                    host_run.append((time.perf_counter() - t0) * 1e3)
                    reduced[:] = host_reduce(measure, h_full.reshape(nw, P), n_rows, n_cols, square, threshold, iu)

                def sweep_call():
                    eng._check(lib.dst_run_windows(eng._h, m, int(square), 0, 1, 0, n_rows, wb.ctypes.data, we.ctypes.data, nw, 0,
                                                   d_out.data_ptr(), d_out.numel() * 8, None))

                def timed(fn):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3

                summary_call()   # warm-up: planes, tables, state
                if host:
                    host_call()
                if baselines:
                    sweep_call()
                host_run.clear()
                a, b, c = [], [], []
                for _ in range(args.steps):   # alternating
                    a.append(timed(summary_call))
                    if host:
                        b.append(timed(host_call))
                    if baselines:
                        c.append(timed(sweep_call))
                if args.kernel_only:
                    continue
                t = np.frombuffer(bytes(tot), np.uint64).reshape(nw, 5)
                out = {"shape": name, "rows": n_rows, "cols": n_cols, "sites": L, "square": square, "windows": nw, "pairs": P,
                       "pair_windows": P * nw, "measure": measure, "threshold": threshold, "steps": args.steps,
                       "per_record": not totals_only, "full_square": "DST_WINDOW_SUMMARY_FULL_SQUARE" in os.environ,
                       "summary_ms": stats(a), "full_result_bytes": nw * P * 8,
                       "summary_result_bytes": nw * 40 + entries * 16, "links": int(t[:, 3].sum()), "nan_pairs": int(t[:, 1].sum())}
                assert (t[:, 0] == P).all()
                if host:
                    h_tot, h_tsum, h_within, h_summable, h_sums = reduced
                    out["same_result"] = bool(
                        np.array_equal(t[:, 1:4], h_tot) and np.array_equal(t[:, 4], h_tsum.view(np.uint64)) and
                        np.array_equal(within.reshape(nw, n_rows), h_within) and np.array_equal(summable.reshape(nw, n_rows), h_summable)
                        and np.array_equal(sums.view(np.uint64).reshape(nw, n_rows), h_sums.view(np.uint64)))
                    out["host_reduce_ms"] = stats(b)
                    out["host_run_ms"] = stats(host_run)
                    out["host_reduce_over_summary"] = round(out["host_reduce_ms"]["median"] / out["summary_ms"]["median"], 2)
                if baselines:
                    out["sweep_ms"] = stats(c)
                    out["summary_over_sweep"] = round(out["summary_ms"]["median"] / out["sweep_ms"]["median"], 2)
                line = json.dumps(out)
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")


if __name__ == "__main__":
    main()
