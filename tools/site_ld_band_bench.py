"""dst_site_ld_links_band / dst_site_ld_decay timing: one JSON line per size on GPU 0, tools/synth alignments.

    python tools/site_ld_band_bench.py [--sizes 10000,50000] [--sites 30000] [--gaps 100,1000,10000] [--bins 100] [--steps 5]
                                       [--r2 0.2] [--out profiles/site_ld/site_ld_band_bench.jsonl]

The listed sites are the variable ones (major base and other bases each held by at least one record, the major base as the
reference allele: `distance --ld`'s list).  Per line, in ONE process and alternating between the calls on every step (one
warm-up of each first), the median, the smallest and the largest of --steps.  These are CALL times (list checks, band plan,
vector build, launches, the wait), not kernel times:
  count_ms          (i) a count-only dst_site_ld_links call at r2 >= --r2 over the whole triangle (the unbanded call);
  band[G].count_ms  (ii) a count-only dst_site_ld_links_band call at max_gap G, beside the band's share of the pairs and of
                    the 64 x 64 tiles (dst_ld_band's `tiles` over the triangle's);
  band[G].decay_ms  (iii) dst_site_ld_decay with --bins bins of width ceil((G + 1) / bins): the same band up to rounding (its
                    own pairs and tiles are given); decay_over_count is its median over the count-only call's at that band;
  whole.decay_ms    (iii) the same call over the whole triangle (one bin width that covers the span);
  host_route        (iv) the route there was before: dst_site_ld's full form into host memory, dst_ld_finalize and a numpy bin
                    reduction (bincount over exact halves of q), on the FIRST `host_listed` listed sites only, the longest
                    prefix whose whole triangle fits one 2^24-pair slab: that is what the route can afford here.  The pair
                    index arrays of the reduction are built once outside the timing.  `decay_ms` is dst_site_ld_decay on the
                    same prefix with the same bins, timed in the same loop, and `same_result` the bitwise comparison of the
                    two curves (pairs, defined, links, r2_sum): the run ends in an error if they differ, or if the whole
                    triangle's links differ from the count-only call's.
A library built with measurement flags is refused."""
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

SLAB_PAIRS = 1 << 24


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def host_curve(eng, sites, alleles, gap, width, bins, min_r2):
    """the curve by the old route: every pair's tallies to the host, r2 there, numpy bins (q summed exactly in two halves)"""
    t, _ = eng.site_ld(sites, alleles)
    r2 = da.ld_finalize(t)["r2"]
    b = gap // width
    ok = (b < bins) & ~np.isnan(r2)
    b, v = b[ok], r2[ok]
    q = np.rint(v * float(1 << da.LD_SCALE_BITS)).astype(np.uint64)
    hi = np.bincount(b, (q >> np.uint64(16)).astype(np.float64), bins).astype(np.uint64)   # (each sum below 2^53: exact)
    lo = np.bincount(b, (q & np.uint64(0xFFFF)).astype(np.float64), bins).astype(np.uint64)
    total = (hi << np.uint64(16)) + lo
    return {"pairs": np.bincount((gap // width)[gap // width < bins], minlength=bins).astype(np.uint64),
            "defined": np.bincount(b, minlength=bins).astype(np.uint64),
            "links": np.bincount(b[v >= min_r2], minlength=bins).astype(np.uint64),
            "r2_sum": total.astype(np.float64) * 2.0 ** -da.LD_SCALE_BITS, "q": total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000")
    ap.add_argument("--sites", type=int, default=30000)
    ap.add_argument("--gaps", default="100,1000,10000")
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--r2", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    flags = da.load().dst_build_flags().decode()
    if flags:
        raise SystemExit(f"libdistance_hip.so was built with measurement flags ({flags}): not a timing build")
    gaps = [int(x) for x in args.gaps.split(",")]
    lines = []
    with da.Engine(0) as eng:
        for n in [int(x) for x in args.sizes.split(",")]:
            codes = synth.alignment(synth.SEED, n, args.sites)
            eng.set_path("dense")   # (every plane stored by the upload: the calls are timed without ensure_planes' one-off work)
            eng.upload(0, codes)
            allele, major, other = da.site_major(eng.site_counts(0))
            sites = np.flatnonzero((major >= 1) & (other >= 1)).astype(np.uint32)
            alleles = np.ascontiguousarray(allele[sites.astype(np.int64)])
            S = len(sites)
            pairs = S * (S - 1) // 2
            span = int(sites[-1] - sites[0])
            _, _, tri_tiles = da.ld_band(sites, span)
            plans = {}
            for G in gaps:
                width = -(-(G + 1) // args.bins)
                plans[G] = {"width": width, "band": da.ld_band(sites, G)[1:], "decay_band": da.ld_band(sites, width * args.bins - 1)[1:]}
            whole_width = -(-(span + 1) // args.bins)
            # (iv): the longest prefix of the list whose triangle is one slab
            K = min(S, int((1 + (1 + 8 * SLAB_PAIRS) ** 0.5) / 2))
            while K * (K - 1) // 2 > SLAB_PAIRS:
                K -= 1
            sub, sub_alleles = sites[:K], alleles[:K]
            i, j = np.triu_indices(K, 1)
            sub_gap = (sub.astype(np.int64)[j] - sub.astype(np.int64)[i])
            del i, j
            sub_width = -(-(int(sub[-1] - sub[0]) + 1) // args.bins)

            calls = {"count": lambda: eng.site_ld_links(sites, args.r2, alleles, count_only=True),
                     "whole_decay": lambda: eng.site_ld_decay(sites, whole_width, args.bins, args.r2, alleles),
                     "host": lambda: host_curve(eng, sub, sub_alleles, sub_gap, sub_width, args.bins, args.r2),
                     "host_decay": lambda: eng.site_ld_decay(sub, sub_width, args.bins, args.r2, sub_alleles)}
            for G in gaps:
                calls[f"band_count_{G}"] = lambda G=G: eng.site_ld_links(sites, args.r2, alleles, count_only=True, max_gap=G)
                calls[f"band_decay_{G}"] = lambda G=G: eng.site_ld_decay(sites, plans[G]["width"], args.bins, args.r2, alleles)
            first = {k: fn() for k, fn in calls.items()}   # warm-ups, and the checks
            same = all(np.array_equal(first["host"][k], first["host_decay"][k]) for k in ("pairs", "defined", "links")) and \
                np.array_equal(first["host"]["r2_sum"].view(np.uint64), first["host_decay"]["r2_sum"].view(np.uint64))
            whole = first["whole_decay"]
            same_whole = int(whole["links"].sum()) == first["count"] and int(whole["pairs"].sum()) == pairs
            if not same or not same_whole:
                raise SystemExit(f"n = {n}: the decay call differs from " + ("the host route's curve" if not same else "the count-only call's links"))
            ms = {k: [] for k in calls}
            for _ in range(args.steps):
                for k, fn in calls.items():
                    ms[k].append(timed(fn)[0])
            med = {k: float(np.median(v)) for k, v in ms.items()}
            line = {"n": n, "sites": args.sites, "listed": S, "pairs": pairs, "span": span, "tiles": tri_tiles, "r2": args.r2,
                    "bins": args.bins, "times": "call times, median/min/max of %d alternating steps" % args.steps,
                    "links": first["count"], "count_ms": stats(ms["count"]), "band": {},
                    "whole": {"width": whole_width, "decay_ms": stats(ms["whole_decay"]),
                              "decay_over_count": round(med["whole_decay"] / med["count"], 3), "links_equal_count": bool(same_whole)},
                    "host_route": {"host_listed": K, "host_pairs": K * (K - 1) // 2, "width": sub_width, "host_ms": stats(ms["host"]),
                                   "decay_ms": stats(ms["host_decay"]), "host_over_decay": round(med["host"] / med["host_decay"], 1),
                                   "same_result": bool(same)}}
            for G in gaps:
                bp, bt = plans[G]["band"]
                dp, dt = plans[G]["decay_band"]
                line["band"][str(G)] = {"pairs": bp, "pair_share": round(bp / pairs, 5), "tiles": bt, "tile_share": round(bt / tri_tiles, 5),
                                        "links": first[f"band_count_{G}"], "count_ms": stats(ms[f"band_count_{G}"]),
                                        "count_over_unbanded": round(med[f"band_count_{G}"] / med["count"], 4),
                                        "decay_width": plans[G]["width"], "decay_pairs": dp, "decay_tiles": dt,
                                        "decay_ms": stats(ms[f"band_decay_{G}"]),
                                        "decay_over_count": round(med[f"band_decay_{G}"] / med[f"band_count_{G}"], 3)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)), exist_ok=True)
        with open(os.path.join(ROOT, args.out), "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
