"""Links streams against the plain stream: one JSON line per measure and stream kind on GPU 0.

    python tools/stream_links_bench.py [--rounds 7] [--batches 20] [--records 1024] [--loaded 50000] [--sites 30000]
                                       [--measures n tn93] [--out profiles/stream_links/stream_links_bench.jsonl]

One process, one session: 50,000 x 30,000 of the tools/synth alignment loaded, --batches batches of --records streamed
records per step (depth 3, the 4-bit wire format, every batch copied into its page-locked ring slot like a caller does).
Per measure five streams over the same batches:
  plain_tally          the plain DST_OUT_TALLY stream, which copies every batch's result matrix back (the yardstick)
  links_sparse         a links stream (DST_LINKS_TALLIES, the default window) at the threshold that links about 1e-4 of
                       the pairs (the 1e-4 quantile of the first batch's distances; the share reached is in the line)
  links_sparse_copy    the same with DST_STREAM_LINKS_COPY: the window in device memory, copied after collect
  links_inf, links_inf_copy   threshold inf: everything that is not NaN links - the wrong tool, its documented cost
Every window of every batch is fetched (dst_stream_links_batch), none is copied again.  After one warm-up round the kinds
take turns, one step each per round, so that drift of the shared host reaches all of them alike; a line holds the median
step, the fastest and the slowest, and streamed records per second at the median.  spread = (max - min) / median of the
yardstick's steps is the session's run-to-run margin.
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

DEPTH = 3


def drain(st):
    """collect the oldest batch; a links stream: fetch every window of it.  Returns the batch's links (0: plain)"""
    if not isinstance(st, da.LinksStream):
        st.pop(copy=False)
        return 0
    n, p = C.c_size_t(), C.c_void_p()
    st._eng._check(st._lib.dst_stream_collect(st._h, C.byref(n), C.byref(p)))
    m, total = C.c_uint64(), C.c_uint64()
    ptr = [C.c_void_p() for _ in range(4)]
    first = 0
    while True:
        st._eng._check(st._lib.dst_stream_links_batch(st._h, first, C.byref(m), C.byref(total), *[C.byref(x) for x in ptr]))
        first += m.value
        if first >= total.value:
            return int(total.value)


def step(st, batches, n_batches):
    links = 0
    for g in range(n_batches):
        b = batches[g % len(batches)]
        if st.in_flight() == st.depth - 1:
            links += drain(st)
        buf, _ = st.buffer()
        buf[:len(b)] = b
        st.submit(len(b))
    while st.in_flight():
        links += drain(st)
    return links


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=5, help="distinct batches generated; a step cycles through them")
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--loaded", type=int, default=50_000)
    ap.add_argument("--sites", type=int, default=30_000)
    ap.add_argument("--measures", nargs="*", default=["n", "tn93"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_links", "stream_links_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    threads = min(len(os.sched_getaffinity(0)), 16)
    B, nb, n_loaded, L = args.records, args.batches, args.loaded, args.sites
    with da.Engine(0) as eng, open(args.out, "a") as out:
        root = synth.root(synth.SEED, L)
        eng.upload(0, synth.records(synth.SEED, root, 0, n_loaded, threads=threads))
        codes = [synth.records(synth.SEED, root, n_loaded + g * B, B, threads=threads) for g in range(args.distinct)]
        batches = [da.engine.Stream.to_nibbles(c) for c in codes]
        for measure in args.measures:
            with eng.stream(measure, B, depth=2) as st:          # the first batch's distances: the 1e-4 quantile
                st.push(codes[0])
                sample = st.pop().reshape(-1).astype(np.float64)
            T = float(np.quantile(sample[np.isfinite(sample)], 1e-4))
            del sample

            def links(threshold, copy):
                if copy:
                    os.environ["DST_STREAM_LINKS_COPY"] = "1"
                try:
                    return eng.links_stream(measure, threshold, B, depth=DEPTH, nibbles=True, values=False, tallies=True)
                finally:
                    os.environ.pop("DST_STREAM_LINKS_COPY", None)

            kinds = [("plain_tally", float("nan"), lambda: eng.stream(measure, B, depth=DEPTH, tallies=True, nibbles=True)),
                     ("links_sparse", T, lambda: links(T, False)), ("links_sparse_copy", T, lambda: links(T, True)),
                     ("links_inf", float("inf"), lambda: links(float("inf"), False)),
                     ("links_inf_copy", float("inf"), lambda: links(float("inf"), True))]
            streams = [(kind, thr, make()) for kind, thr, make in kinds]
            times = {kind: [] for kind, _, _ in kinds}
            found = {}
            try:
                for r in range(args.rounds + 1):                 # round 0 warms every stream's slots and kernels up
                    for kind, _, st in streams:
                        t0 = time.perf_counter()
                        found[kind] = step(st, batches, nb)
                        if r:
                            times[kind].append(time.perf_counter() - t0)
                stats = {kind: (st.stats() if isinstance(st, da.LinksStream) else (0, 0)) for kind, _, st in streams}
            finally:
                for _, _, st in streams:
                    st.close()
            base = times["plain_tally"]
            spread = (max(base) - min(base)) / float(np.median(base))
            for kind, thr, _ in kinds:
                t = times[kind]
                el = float(np.median(t))
                line = json.dumps({"stream": kind, "measure": measure, "loaded": n_loaded, "sites": L, "batch_records": B,
                                   "batches_per_step": nb, "depth": DEPTH, "wire": "nibbles", "rounds": args.rounds,
                                   "threshold": None if thr != thr else repr(thr), "links_per_step": found[kind],
                                   "link_share": found[kind] / float(nb * B * n_loaded),
                                   "late_windows_total": stats[kind][1],
                                   "ms_per_step": round(el * 1e3, 3), "ms_min": round(min(t) * 1e3, 3),
                                   "ms_max": round(max(t) * 1e3, 3), "streamed_records_per_s": nb * B / el,
                                   "vs_plain": float(np.median(base)) / el, "plain_spread": round(spread, 4),
                                   "path": eng.last_path()})
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
