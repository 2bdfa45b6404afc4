"""dst_run_windows timing: one JSON line per (shape, measure) on GPU 0, tools/synth alignments.

    python tools/windows_bench.py [--shape scan|genes|both] [--measures n,tn93] [--steps 5]
                                  [--out profiles/windows/windows_bench.jsonl] [--kernel-only]

Shapes: `scan`, 16 queries x 10,000 records x 30,000 sites with the windows of `--windows 1000 --step 200` (146 of
them), a rectangle; `genes`, the square of 2,000 x 30,000 with 12 regions.  Per line, in ONE process and alternating
between the two variants on every step (one warm-up of each first), the median, the smallest and the largest of --steps:
  windows_ms     (a) one dst_run_windows call into device memory, DST_OUT_DISTANCE, the call's own wait included;
  windows_dev_ms     the same call's work on the device, between two events on the caller's stream: the window table's
                     copy, tn93's count kernel(s) and the pair kernel (rocprofv3 --kernel-trace --stats, with
                     --kernel-only in a run of its own, gives the kernels apart);
  per_window_ms  (b) the same answer the way it was had without dst_run_windows: per window the columns cut on the host,
                     dst_upload of both sets on a second context, dst_run_rect / dst_run_square into device memory; the
                     results of the two variants are compared bitwise at the timed size (`same_bits`);
  dense_pair_ms      the dense pair kernel over the FULL width for the same pairs (DST_PATH_DENSE, the library's own
                     events around the kernel), for its rate in site comparisons per second;
and from them: the ratio (b) / (a), the window kernel's rate = pairs x the windows' total sites / windows_dev_ms, the
dense kernel's rate = pairs x sites / dense_pair_ms, and what a store-bound model gives for the output bytes at the
--fill-TBps rate (default 4.7, README's plain-fill figure)."""
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
from tools import synth  # noqa: E402

GENES = [(265, 21555), (265, 13468), (13467, 21555), (21562, 25384), (25392, 26220), (26244, 26472), (26522, 27191),
         (27201, 27387), (27393, 27759), (27893, 28259), (28273, 29533), (55, 29803)]   # 0-based [begin, end)


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["scan", "genes", "both"])
    ap.add_argument("--measures", default="n,tn93")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--fill-TBps", type=float, default=4.7)
    ap.add_argument("--kernel-only", action="store_true", help="only the dst_run_windows calls (for a profiler's run)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    lib = da.load()
    L = 30_000
    shapes = []
    if args.shape in ("scan", "both"):
        shapes.append(("scan", 16, 10_000, da.sliding_windows(L, 1000, 200)))
    if args.shape in ("genes", "both"):
        shapes.append(("genes", 2_000, 2_000, np.array(GENES, np.uint64)))
    for name, n_rows, n_cols, windows in shapes:
        square = name == "genes"
        cols = synth.alignment(synth.SEED, n_cols, L)
        rows = cols if square else synth.alignment(synth.SEED ^ 1, n_rows, L)
        nw = len(windows)
        wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
        P = n_cols * (n_cols - 1) // 2 if square else n_rows * n_cols
        site_sum = int((we - wb).sum())
        with da.Engine(0) as eng, da.Engine(0) as cut:
            eng.set_path("dense")   # (the whole-width yardstick is the dense kernel; dst_run_windows does not look at the path)
            if square:
                eng.upload(0, cols)
            else:
                eng.upload(0, rows)
                eng.upload(1, cols)
            stream = torch.cuda.Stream()
            for measure in args.measures.split(","):
                m = da.MEASURES[measure]
                d_out = torch.zeros(nw * P, dtype=torch.float64, device="cuda")
                d_one = torch.zeros(nw * P, dtype=torch.float64, device="cuda")
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                def windows_call(handle=None):
                    eng._check(lib.dst_run_windows(eng._h, m, int(square), 0, 1, 0, n_rows, wb.ctypes.data, we.ctypes.data, nw, 0,
                                                   d_out.data_ptr(), d_out.numel() * 8, handle))

                def windows_device_ms():
                    with torch.cuda.stream(stream):
                        ev0.record(stream)
                        windows_call(stream.cuda_stream)
                        ev1.record(stream)
                    ev1.synchronize()
                    return ev0.elapsed_time(ev1)

                def per_window():
                    for w in range(nw):
                        lo, hi = int(wb[w]), int(we[w])
                        at = d_one.data_ptr() + w * P * 8
                        if square:
                            cut.upload(0, np.ascontiguousarray(cols[:, lo:hi]))
                            cut.run_square_device(measure, 0, n_cols, at, P * 8)
                        else:
                            cut.upload(0, np.ascontiguousarray(rows[:, lo:hi]))
                            cut.upload(1, np.ascontiguousarray(cols[:, lo:hi]))
                            cut.run_rect_device(measure, 0, 1, 0, n_rows, at, P * 8)

                def timed(fn):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3

                windows_call()   # warm-up: planes, tables
                if args.kernel_only:
                    for _ in range(args.steps):
                        windows_call()
                    continue
                per_window()
                a, a_dev, b = [], [], []
                for _ in range(args.steps):   # alternating
                    a.append(timed(windows_call))
                    b.append(timed(per_window))
                    a_dev.append(windows_device_ms())
                got, want = d_out.cpu().numpy().view(np.uint64), d_one.cpu().numpy().view(np.uint64)
                nan = np.isnan(got.view(np.float64)) & np.isnan(want.view(np.float64)) if measure not in da.INT_MEASURES else False
                same = bool(((got == want) | nan).all())
                dense = []
                d_full = torch.zeros(P, dtype=torch.float64, device="cuda")
                for _ in range(args.steps + 1):
                    if square:
                        eng.run_square_device(measure, 0, n_cols, d_full.data_ptr(), P * 8)
                    else:
                        eng.run_rect_device(measure, 0, 1, 0, n_rows, d_full.data_ptr(), P * 8)
                    dense.append(eng.last_kernel_ms()["pair_ms"])
                dense = dense[1:]
                out_bytes = nw * P * 8
                a_s, d_s, b_s, k_s = stats(a), stats(a_dev), stats(b), stats(dense)
                line = json.dumps({
                    "shape": name, "rows": n_rows, "cols": n_cols, "sites": L, "square": square, "windows": nw,
                    "window_sites_total": site_sum, "pairs": P, "measure": measure, "steps": args.steps, "same_bits": same,
                    "windows_ms": a_s, "windows_dev_ms": d_s, "per_window_ms": b_s, "dense_pair_ms": k_s,
                    "per_window_over_windows": round(b_s["median"] / a_s["median"], 2),
                    "window_rate_site_cmp_per_s": float(f"{P * site_sum / (d_s['median'] * 1e-3):.4g}"),
                    "dense_rate_site_cmp_per_s": float(f"{P * L / (k_s['median'] * 1e-3):.4g}"),
                    "out_bytes": out_bytes, "store_model_ms": round(out_bytes / (args.fill_TBps * 1e12) * 1e3, 3),
                })
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")


if __name__ == "__main__":
    main()
