"""dst_site_ld / dst_site_ld_links timing: one JSON line per (size, minimum count) on GPU 0, tools/synth
alignments.

    python tools/site_ld_bench.py [--sizes 10000,50000] [--sites 30000] [--counts 1,10] [--steps 5] [--r2 0.2]
                                  [--host-rows 2] [--out profiles/site_ld/site_ld_bench.jsonl]

The listed sites are the variable ones: those whose major base and whose other bases together are each held by at least C
records (Engine.site_counts + site_major, as `distance --ld --ld-min-count C` lists them), with the major base as the
reference allele.  Per line, in ONE process and alternating between the calls on every step (one warm-up of each first),
the median, the smallest and the largest of --steps:
  count_ms   a count-only dst_site_ld_links call at r2 >= --r2 over all pairs of listed sites;
  links_ms   the same call with a sink (the links copied out; left out, null, above 50 million links);
  dense_ms   dst_site_ld for the first row slab (the leading rows that hold at most 2^24 pairs);
  host_ms    (a) the only route there was before: the same tallies on the host from np.packbits bit vectors, AND and a byte
                 popcount table, for the first --host-rows rows against every later site, compared bitwise with the
                 library's in the same run (`same_result`); host_scaled_ms is that time times (all pairs / those rows'
                 pairs): a SCALED figure, not a measurement of the whole triangle; host_build_ms, the bit vectors of the
                 whole list (once, not scaled), comes on top.
and beside them floor_ms, (b): 8 v_and_b32 and 8 v_bcnt_u32_b32 per pair and 64 records at the issue rates tools/ubench
measured at 4 waves per SIMD (profiles/r01/ubench_valu_rate.txt: 1.057 and 1.837 ns per wave instruction and SIMD) on 1,024
SIMDs: COMPUTED from the shape, not measured.  A library built with measurement flags is refused."""
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
from tools import synth  # noqa: E402

AND_NS, BCNT_NS, SIMDS = 1.057, 1.837, 1024
SLAB_PAIRS = 1 << 24
MAX_LINKS_OUT = 50_000_000   # more links than this: the call with a sink is left out (links_ms null)
CLASS = np.full(16, 255, np.uint8)
CLASS[[0b1000, 0b0001, 0b0100, 0b0010]] = [0, 1, 2, 3]
POP8 = np.array([bin(x).count("1") for x in range(256)], np.uint8)
COLUMN_BLOCK = 512


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def host_vectors(codes, sites, alleles):
    """(C, M): uint8[S, ceil(n / 8)] bit vectors along the records"""
    C, M = [], []
    for b in range(0, len(sites), COLUMN_BLOCK):
        cls = CLASS[codes[:, sites[b:b + COLUMN_BLOCK]] >> 4]
        called = cls < 4
        C.append(np.packbits(called.T, axis=1))
        M.append(np.packbits((called & (cls != alleles[None, b:b + COLUMN_BLOCK])).T, axis=1))
    return np.concatenate(C), np.concatenate(M)


def host_rows(C, M, rows):
    """the tallies of rows [0, rows) against every later position, canonical order"""
    out = []
    for p in range(rows):
        cq, mq = C[p + 1:], M[p + 1:]
        out.append(np.stack([POP8[C[p] & cq].sum(axis=1, dtype=np.uint32), POP8[M[p] & cq].sum(axis=1, dtype=np.uint32), POP8[C[p] & mq].sum(axis=1, dtype=np.uint32),
                             POP8[M[p] & mq].sum(axis=1, dtype=np.uint32)], axis=1))
    return np.concatenate(out).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000")
    ap.add_argument("--sites", type=int, default=30000)
    ap.add_argument("--counts", default="1,10")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--r2", type=float, default=0.2)
    ap.add_argument("--host-rows", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    flags = da.load().dst_build_flags().decode()
    if flags:
        raise SystemExit(f"libdistance_hip.so was built with measurement flags ({flags}): not a timing build")
    lines = []
    with da.Engine(0) as eng:
        for n in [int(x) for x in args.sizes.split(",")]:
            codes = synth.alignment(synth.SEED, n, args.sites)
            eng.set_path("dense")   # (every plane stored by the upload: the calls are timed without ensure_planes' one-off work)
            eng.upload(0, codes)
            allele, major, other = da.site_major(eng.site_counts(0))
            for c in [int(x) for x in args.counts.split(",")]:
                sites = np.flatnonzero((major >= c) & (other >= c)).astype(np.uint32)
                alleles = np.ascontiguousarray(allele[sites.astype(np.int64)])
                S = len(sites)
                if S < 2:
                    continue
                pairs = S * (S - 1) // 2
                rows, slab_pairs = 0, 0
                while rows < S and slab_pairs + (S - rows - 1) <= SLAB_PAIRS:
                    slab_pairs += S - rows - 1
                    rows += 1
                rows = max(rows, 1)
                hr = min(args.host_rows, rows)
                words = (n + 63) // 64
                floor_ms = pairs * words / 64 * 8 * (AND_NS + BCNT_NS) / SIMDS * 1e-6   # (a wave instruction serves 64 pairs)
                n_links = eng.site_ld_links(sites, args.r2, alleles, count_only=True)   # warm-ups, and the check
                full = n_links <= MAX_LINKS_OUT   # (the links are copied into numpy arrays: 24 bytes each)
                got = eng.site_ld_links(sites, args.r2, alleles) if full else None
                dense, _ = eng.site_ld(sites, alleles, row_end=rows)
                t0 = time.perf_counter()
                C, M = host_vectors(codes, sites, alleles)
                build_ms = (time.perf_counter() - t0) * 1e3
                want = host_rows(C, M, hr)
                same = bool(np.array_equal(dense[:len(want)], want)) and (not full or len(got[0]) == n_links)
                count, links, dns, host = [], [], [], []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    eng.site_ld_links(sites, args.r2, alleles, count_only=True)
                    count.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    if full:
                        eng.site_ld_links(sites, args.r2, alleles)
                        links.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    eng.site_ld(sites, alleles, row_end=rows)
                    dns.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    host_rows(C, M, hr)
                    host.append((time.perf_counter() - t0) * 1e3)
                host_pairs = len(want)
                line = {"n": n, "sites": args.sites, "min_count": c, "listed": S, "pairs": pairs, "r2": args.r2, "links": n_links,
                        "count_ms": stats(count), "links_ms": stats(links) if full else None, "dense_rows": rows, "dense_pairs": slab_pairs,
                        "dense_ms": stats(dns), "floor_ms": round(floor_ms, 3), "floor": "computed, not measured",
                        "count_over_floor": round(float(np.median(count)) / floor_ms, 2), "host_rows": hr, "host_pairs": host_pairs,
                        "host_ms": stats(host), "host_build_ms": round(build_ms, 1),
                        "host_scaled_ms": round(float(np.median(host)) * pairs / host_pairs, 1), "host_scaled": "scaled by the pair ratio",
                        "host_scaled_over_count": round(float(np.median(host)) * pairs / host_pairs / float(np.median(count)), 1),
                        "same_result": same}
                print(json.dumps(line), flush=True)
                lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)), exist_ok=True)
        with open(os.path.join(ROOT, args.out), "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
