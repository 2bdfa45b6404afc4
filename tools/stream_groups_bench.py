"""Group-summary streams against the plain distance stream and the summary stream: one JSON line per measure
and leg on GPU 0.

    python tools/stream_groups_bench.py [--rounds 5] [--batches 20] [--records 1024] [--loaded 50000] [--sites 30000]
                                        [--measures n tn93] [--legs ...] [--out profiles/stream_groups/stream_groups_bench.jsonl]

One process, one session: 50,000 x 30,000 of the tools/synth alignment loaded, --batches batches of --records streamed
records per step (depth 3, the 4-bit wire format, every batch and its labels copied into the page-locked ring slot like a
caller does).  Per measure, over the same batches:
  (a) plain_numpy       the plain DST_OUT_DISTANCE stream with every batch's matrix reduced by label in numpy on the host: the
                        only way before.  Its result is compared bitwise (min / max as numbers) with one step of a fresh
                        group-summary stream in the same run (`numpy_equal` in its line); --numpy-rounds rounds (default 1)
      plain_distance    the plain stream alone, which copies every batch's matrix back
  (b) summary_loaded, summary_both   the summary stream: the same pass without keys
  (c) the group-summary stream, G_s = 3 unless said otherwise, streamed record r in group r mod G_s:
      cells_3c / cells_3i / cells_1000            cells only; 3 contiguous loaded groups, 3 interleaved record by record, 1,000
      streamed_3c / streamed_3i / streamed_1000   ... with DST_STREAM_GROUPS_STREAMED, every batch's table fetched
      loaded_3 / loaded_1000                      DST_STREAM_GROUPS_LOADED with 3 and 1,000 streamed groups (3 contiguous
                                                  loaded groups)
The threshold is the median of the first batch's distances.  A kept-state leg keeps one stream for all its rounds and takes a
snapshot (result()) at the end of every step, inside the step's time (`snapshot_ms`: its share; with LOADED it copies and
converts 24 bytes per (loaded record, streamed group)).  After one warm-up round the GPU legs take turns, one
step each per round, so that drift of the shared host reaches all of them alike; a line holds the median step, the fastest
and the slowest, streamed records per second at the median and the ratios to (a) and to (b) (summary_loaded).
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
GROUP_LEGS = {  # leg: (loaded layout, G_l, G_s, loaded, streamed)
    "cells_3c": ("contiguous", 3, 3, False, False), "cells_3i": ("interleaved", 3, 3, False, False),
    "cells_1000": ("contiguous", 1000, 3, False, False),
    "streamed_3c": ("contiguous", 3, 3, False, True), "streamed_3i": ("interleaved", 3, 3, False, True),
    "streamed_1000": ("contiguous", 1000, 3, False, True),
    "loaded_3": ("contiguous", 3, 3, True, False), "loaded_1000": ("contiguous", 3, 1000, True, False),
}
LEGS = ("plain_distance", "summary_loaded", "summary_both") + tuple(GROUP_LEGS) + ("plain_numpy",)


def loaded_labels(n, G, layout):
    r = np.arange(n, dtype=np.int64)
    return ((r * G) // n if layout == "contiguous" else r % G).astype(np.uint32)


class NumpyGroups:
    """dst_group_summary's definition on the host, batch by batch, for contiguous loaded groups: integer accumulators, one
    conversion at the end"""

    def __init__(self, measure, lg, Gl, Gs, threshold):
        self.int_payload = measure in da.INT_MEASURES
        self.T = math.floor(threshold) if self.int_payload else threshold
        assert (np.diff(lg.astype(np.int64)) >= 0).all()
        self.starts = np.searchsorted(lg, np.arange(Gl))
        self.sizes = np.bincount(lg, minlength=Gl).astype(np.int64)
        self.Gl, self.Gs, self.n = Gl, Gs, len(lg)
        self.cell = np.zeros((4, Gs, Gl), np.int64)              # nan, summable, links, q
        self.kmin = np.full((Gs, Gl), np.inf)
        self.kmax = np.full((Gs, Gl), -np.inf)
        self.rec = np.zeros((3, self.n, Gs), np.int64)           # within, summable, q of (loaded record, streamed group)
        self.rows = np.zeros(Gs, np.int64)
        self.streamed = []

    def add(self, S, sg):
        if self.int_payload:
            ok, q, nan = np.ones(S.shape, bool), S, np.zeros(S.shape, bool)
        else:
            with np.errstate(invalid="ignore"):
                ok = np.abs(S) < 2.0 ** 25
            q = np.rint(np.where(ok, S, 0.0) * 2.0 ** 37).astype(np.int64)
            nan = np.isnan(S)
        with np.errstate(invalid="ignore"):
            link = S <= self.T
        per = [np.add.reduceat(x, self.starts, axis=1, dtype=np.int64) for x in (nan, ok, link, q)]   # (B, Gl) each
        lo = np.fmin.reduceat(S.astype(np.float64), self.starts, axis=1)
        hi = np.fmax.reduceat(S.astype(np.float64), self.starts, axis=1)
        self.streamed.append((per[2].astype(np.uint32), per[1].astype(np.uint32), self.convert(per[3])))
        for a in range(self.Gs):
            rows = sg == a
            if not rows.any():
                continue
            self.rows[a] += int(rows.sum())
            for k in range(4):
                self.cell[k, a] += per[k][rows].sum(axis=0)
            self.kmin[a] = np.fmin(self.kmin[a], np.fmin.reduce(lo[rows], axis=0))
            self.kmax[a] = np.fmax(self.kmax[a], np.fmax.reduce(hi[rows], axis=0))
            for k, x in enumerate((link, ok, q)):
                self.rec[k, :, a] += x[rows].sum(axis=0, dtype=np.int64)

    def convert(self, sums):
        vals = np.array([float(int(s)) for s in sums.reshape(-1)], np.float64)
        return (vals if self.int_payload else np.ldexp(vals, -37)).reshape(sums.shape)

    def equals(self, res, streamed):
        pairs = np.outer(self.rows, self.sizes)
        known = pairs > self.cell[0]
        same = (np.array_equal(res["pairs"], pairs.astype(np.uint64)) and np.array_equal(res["nan_pairs"], self.cell[0].astype(np.uint64))
                and np.array_equal(res["summable_pairs"], self.cell[1].astype(np.uint64))
                and np.array_equal(res["links"], self.cell[2].astype(np.uint64))
                and np.array_equal(res["sum"].view(np.uint64), self.convert(self.cell[3]).view(np.uint64))
                and np.array_equal(res["min"][known].astype(np.float64), self.kmin[known])
                and np.array_equal(res["max"][known].astype(np.float64), self.kmax[known])
                and np.array_equal(res["rec_within"], self.rec[0].astype(np.uint32))
                and np.array_equal(res["rec_summable"], self.rec[1].astype(np.uint32))
                and np.array_equal(res["rec_sum"].view(np.uint64), self.convert(self.rec[2]).view(np.uint64)))
        mine = [np.concatenate([b[a] for b in self.streamed]) for a in range(3)]
        return bool(same and all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(m).view(np.uint8))
                                 for g, m in zip(streamed, mine)))


def step(st, batches, n_batches, labels=None, sink=None):
    """one step: n_batches batches through the stream; labels[g]: the batch's streamed labels (a group-summary stream);
    sink(batch number, what pop returned) per batch"""
    popped = 0
    for g in range(n_batches):
        b = batches[g % len(batches)]
        if st.in_flight() == st.depth - 1:
            got = st.pop(copy=False)
            if sink:
                sink(popped, got)
            popped += 1
        buf, _ = st.buffer()
        buf[:len(b)] = b
        if labels is not None:
            st.labels()[:len(b)] = labels[g % len(labels)]
        st.submit(len(b))
    while st.in_flight():
        got = st.pop(copy=False)
        if sink:
            sink(popped, got)
        popped += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--numpy-rounds", type=int, default=1)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=5, help="distinct batches generated; a step cycles through them")
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--loaded", type=int, default=50_000)
    ap.add_argument("--sites", type=int, default=30_000)
    ap.add_argument("--measures", nargs="*", default=["n", "tn93"])
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_groups", "stream_groups_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    threads = min(len(os.sched_getaffinity(0)), 16)
    B, nb, n_loaded, L = args.records, args.batches, args.loaded, args.sites
    with da.Engine(0) as eng, open(args.out, "a") as out:
        root = synth.root(synth.SEED, L)
        eng.upload(0, synth.records(synth.SEED, root, 0, n_loaded, threads=threads))
        codes = [synth.records(synth.SEED, root, n_loaded + g * B, B, threads=threads) for g in range(args.distinct)]
        batches = [da.engine.Stream.to_nibbles(c) for c in codes]
        streamed_labels = {Gs: [((np.arange(B) + g * B) % Gs).astype(np.uint32) for g in range(args.distinct)] for Gs in (3, 1000)}
        for measure in args.measures:
            with eng.stream(measure, B, depth=2) as st:          # the first batch's distances: their median
                st.push(codes[0])
                sample = st.pop().reshape(-1).astype(np.float64)
            T = float(np.median(sample[np.isfinite(sample)]))
            del sample

            def groups(layout, Gl, Gs, loaded, streamed):
                return eng.group_summary_stream(measure, B, loaded_groups=loaded_labels(n_loaded, Gl, layout), n_loaded_groups=Gl,
                                                n_streamed_groups=Gs, threshold=T, loaded=loaded, streamed=streamed, depth=DEPTH,
                                                nibbles=True)

            kinds = [("plain_distance", lambda: eng.stream(measure, B, depth=DEPTH, nibbles=True)),
                     ("summary_loaded", lambda: eng.summary_stream(measure, B, threshold=T, depth=DEPTH, nibbles=True)),
                     ("summary_both", lambda: eng.summary_stream(measure, B, threshold=T, streamed=True, depth=DEPTH, nibbles=True))]
            kinds += [(leg, lambda cfg=cfg: groups(*cfg)) for leg, cfg in GROUP_LEGS.items()]
            streams = [(kind, make()) for kind, make in kinds if kind in args.legs]
            times = {kind: [] for kind, _ in streams}
            snaps = {kind: [] for kind, _ in streams}            # the snapshot's share of each step
            try:
                for r in range(args.rounds + 1):                 # round 0 warms every stream's slots and kernels up
                    for kind, st in streams:
                        lab = streamed_labels[st.n_streamed_groups] if isinstance(st, da.GroupSummaryStream) else None
                        t0 = time.perf_counter()
                        step(st, batches, nb, lab)
                        t1 = time.perf_counter()
                        if hasattr(st, "result"):                # (a snapshot of everything so far)
                            st.result()
                        if r:
                            times[kind].append(time.perf_counter() - t0)
                            snaps[kind].append(time.perf_counter() - t1)
            finally:
                for _, st in streams:
                    st.close()
            numpy_equal = None
            if "plain_numpy" in args.legs:
                # one step's own answer, from a fresh stream with both tables: what the numpy leg is compared with
                got = []
                with groups("contiguous", 3, 3, True, True) as st:
                    step(st, batches, nb, streamed_labels[3], lambda k, x: got.append(tuple(np.array(a) for a in x[1:])))
                    one_step = st.result()
                side = [np.concatenate([g[a] for g in got]) for a in range(3)]
                times["plain_numpy"] = []
                for _ in range(args.numpy_rounds):
                    ref = NumpyGroups(measure, loaded_labels(n_loaded, 3, "contiguous"), 3, 3, T)
                    with eng.stream(measure, B, depth=DEPTH, nibbles=True) as st:
                        t0 = time.perf_counter()
                        step(st, batches, nb, None, lambda k, S: ref.add(S, streamed_labels[3][k % args.distinct]))
                        times["plain_numpy"].append(time.perf_counter() - t0)
                numpy_equal = ref.equals(one_step, side)
            a_leg, b_leg = times.get("plain_numpy"), times.get("summary_loaded")
            for kind in args.legs:
                t = times.get(kind)
                if not t:
                    continue
                el = float(np.median(t))
                cfg = GROUP_LEGS.get(kind)
                line = json.dumps({"leg": kind, "measure": measure, "loaded": n_loaded, "sites": L, "batch_records": B,
                                   "batches_per_step": nb, "depth": DEPTH, "wire": "nibbles", "rounds": len(t), "threshold": repr(T),
                                   "loaded_layout": cfg[0] if cfg else None, "loaded_groups": cfg[1] if cfg else None,
                                   "streamed_groups": cfg[2] if cfg else None,
                                   "ms_per_step": round(el * 1e3, 3), "ms_min": round(min(t) * 1e3, 3),
                                   "ms_max": round(max(t) * 1e3, 3), "spread": round((max(t) - min(t)) / el, 4),
                                   "snapshot_ms": round(float(np.median(snaps[kind])) * 1e3, 3) if snaps.get(kind) else None,
                                   "streamed_records_per_s": nb * B / el,
                                   "vs_plain_numpy": float(np.median(a_leg)) / el if a_leg else None,
                                   "vs_summary_loaded": float(np.median(b_leg)) / el if b_leg else None,
                                   "numpy_equal": numpy_equal if kind == "plain_numpy" else None, "path": eng.last_path()})
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
