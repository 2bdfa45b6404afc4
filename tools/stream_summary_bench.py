"""Summary streams against the plain distance stream: one JSON line per measure and leg on GPU 0.

    python tools/stream_summary_bench.py [--rounds 7] [--batches 20] [--records 1024] [--loaded 50000] [--sites 30000]
                                         [--measures n tn93] [--legs ...] [--out profiles/stream_summary/stream_summary_bench.jsonl]

One process, one session: 50,000 x 30,000 of the tools/synth alignment loaded, --batches batches of --records streamed
records per step (depth 3, the 4-bit wire format, every batch copied into its page-locked ring slot like a caller does).
Per measure five legs over the same batches:
  plain_distance        the plain DST_OUT_DISTANCE stream, which copies every batch's result matrix back (the yardstick)
  summary_loaded        a summary stream with DST_STREAM_SUMMARY_LOADED
  summary_both          ... with LOADED | STREAMED, every batch's streamed side fetched
  summary_both_hist     ... and 256 bins
  plain_numpy           the plain stream with every batch reduced by numpy on the host: the only way before.  Its result is
                        compared bitwise with one step of a fresh summary stream in the same run (`numpy_equal` in its
                        line); it runs --numpy-rounds rounds (default 1, no warm-up of its own: the reduction dwarfs
                        everything else)
The threshold is the median of the first batch's distances.  A summary leg keeps one stream for all its rounds and takes a
snapshot (result()) at the end of every step, inside the step's time.  After one warm-up round the GPU legs take turns, one
step each per round, so that drift of the shared host reaches all of them alike; a line holds the median step, the fastest and the
slowest, and streamed records per second at the median.  spread = (max - min) / median of a leg's own steps is its
run-to-run margin: "no slower than the yardstick" means inside the two legs' spreads.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402

DEPTH = 3
BINS = 256
LEGS = ("plain_distance", "summary_loaded", "summary_both", "summary_both_hist", "plain_numpy")


class NumpySummary:
    """dst_summary's definition on the host, batch by batch: integer accumulators, one conversion at the end"""

    def __init__(self, measure, n_loaded, threshold):
        self.int_payload = measure in da.INT_MEASURES
        self.T = math.floor(threshold) if self.int_payload else threshold
        self.within = np.zeros(n_loaded, np.int64)
        self.summable = np.zeros(n_loaded, np.int64)
        self.q = np.zeros(n_loaded, np.int64)
        self.streamed = []
        self.nan = 0

    def add(self, S):
        if self.int_payload:
            ok, q = None, S
        else:
            with np.errstate(invalid="ignore"):
                ok = np.abs(S) < 2.0 ** 25
            q = np.rint(np.where(ok, S, 0.0) * 2.0 ** 37).astype(np.int64)
            self.nan += int(np.isnan(S).sum())
        with np.errstate(invalid="ignore"):
            link = S <= self.T
        self.within += link.sum(axis=0)
        self.summable += S.shape[0] if ok is None else ok.sum(axis=0)
        self.q += q.sum(axis=0, dtype=np.int64)
        self.streamed.append((link.sum(axis=1).astype(np.uint32),
                              np.full(S.shape[0], S.shape[1], np.uint32) if ok is None else ok.sum(axis=1).astype(np.uint32),
                              self.convert(q.sum(axis=1, dtype=np.int64))))

    def convert(self, sums):
        vals = [float(int(s)) for s in sums]
        return np.array(vals if self.int_payload else [math.ldexp(v, -37) for v in vals], np.float64)

    def equals(self, result, streamed):
        mine = [np.concatenate([b[a] for b in self.streamed]) for a in range(3)]
        same = (np.array_equal(result["within"], self.within.astype(np.uint32))
                and np.array_equal(result["summable"], self.summable.astype(np.uint32))
                and np.array_equal(result["sum"].view(np.uint64), self.convert(self.q).view(np.uint64))
                and result["nan_pairs"] == self.nan and result["links"] == int(self.within.sum())
                and result["summable_pairs"] == int(self.summable.sum()))
        return bool(same and all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(m).view(np.uint8))
                                 for g, m in zip(streamed, mine)))


def step(st, batches, n_batches, sink=None):
    """one step: n_batches batches through the stream; sink(what pop returned) per batch"""
    for g in range(n_batches):
        b = batches[g % len(batches)]
        if st.in_flight() == st.depth - 1:
            got = st.pop(copy=False)
            if sink:
                sink(got)
        buf, _ = st.buffer()
        buf[:len(b)] = b
        st.submit(len(b))
    while st.in_flight():
        got = st.pop(copy=False)
        if sink:
            sink(got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--numpy-rounds", type=int, default=1)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=5, help="distinct batches generated; a step cycles through them")
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--loaded", type=int, default=50_000)
    ap.add_argument("--sites", type=int, default=30_000)
    ap.add_argument("--measures", nargs="*", default=["n", "tn93"])
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_summary", "stream_summary_bench.jsonl"))
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
            with eng.stream(measure, B, depth=2) as st:          # the first batch's distances: their median
                st.push(codes[0])
                sample = st.pop().reshape(-1).astype(np.float64)
            T = float(np.median(sample[np.isfinite(sample)]))
            width = max(1.0, math.floor(T / 64)) if measure in da.INT_MEASURES else T / 128
            del sample

            def summary(loaded, streamed, bins):
                return eng.summary_stream(measure, B, threshold=T, loaded=loaded, streamed=streamed, bins=bins, width=width,
                                          depth=DEPTH, nibbles=True)

            kinds = [("plain_distance", lambda: eng.stream(measure, B, depth=DEPTH, nibbles=True)),
                     ("summary_loaded", lambda: summary(True, False, 0)), ("summary_both", lambda: summary(True, True, 0)),
                     ("summary_both_hist", lambda: summary(True, True, BINS))]
            streams = [(kind, make()) for kind, make in kinds if kind in args.legs]
            times = {kind: [] for kind, _ in streams}
            try:
                for r in range(args.rounds + 1):                 # round 0 warms every stream's slots and kernels up
                    for kind, st in streams:
                        t0 = time.perf_counter()
                        step(st, batches, nb)
                        if isinstance(st, da.SummaryStream):     # (a snapshot of everything so far: O(n_loaded + bins))
                            st.result()
                        if r:
                            times[kind].append(time.perf_counter() - t0)
            finally:
                for _, st in streams:
                    st.close()
            # one step's own answer, from a fresh stream with everything asked for: what the numpy leg is compared with
            got = []
            with summary(True, True, BINS) as st:
                step(st, batches, nb, got.append)
                one_step = st.result()
            side = [np.concatenate([g[a] for g in got]) for a in (1, 2, 3)]
            numpy_equal = None
            if "plain_numpy" in args.legs:
                times["plain_numpy"] = []
                for _ in range(args.numpy_rounds):
                    ref = NumpySummary(measure, n_loaded, T)
                    with eng.stream(measure, B, depth=DEPTH, nibbles=True) as st:
                        t0 = time.perf_counter()
                        step(st, batches, nb, ref.add)
                        times["plain_numpy"].append(time.perf_counter() - t0)
                numpy_equal = ref.equals(one_step, side)
            base = times.get("plain_distance")
            for kind in args.legs:
                t = times.get(kind)
                if not t:
                    continue
                el = float(np.median(t))
                line = json.dumps({"leg": kind, "measure": measure, "loaded": n_loaded, "sites": L, "batch_records": B,
                                   "batches_per_step": nb, "depth": DEPTH, "wire": "nibbles", "rounds": len(t),
                                   "threshold": repr(T), "bins": BINS if kind == "summary_both_hist" else 0,
                                   "links_per_step": one_step["links"], "nan_pairs_per_step": one_step["nan_pairs"],
                                   "ms_per_step": round(el * 1e3, 3), "ms_min": round(min(t) * 1e3, 3),
                                   "ms_max": round(max(t) * 1e3, 3), "spread": round((max(t) - min(t)) / el, 4),
                                   "streamed_records_per_s": nb * B / el,
                                   "vs_plain": float(np.median(base)) / el if base else None,
                                   "numpy_equal": numpy_equal if kind == "plain_numpy" else None, "path": eng.last_path()})
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
