"""bench.py --workload C4: BASELINE.json configs[3] — 1,000 x 5,000,000 bp loaded (resident, packed once) against
streamed batches, -m n_high.  The 100,000-record stream (500 GB encoded) is never materialised: a step is a fixed
number of batches synthesised in page-locked host memory by SURVEY 8(d)'s generator before the timed region.

Two figures, the second with --full only:
  value / device_resident   batches already in HBM: pack + compare per batch (inputs resident when timing starts)
  h2d_inclusive             the same batches from page-locked host memory through the overlapped pipeline
                            (dst_stream_*: H2D of batch k+1 and D2H of batch k-1 under the compare of batch k), for both
                            wire formats (Paradis bytes; the codes' high nibbles, two sites per byte), with the ring
                            slots filled in place — what a parser that encodes straight into the slot leaves behind —
                            and, apart, with a host memcpy of every batch into its slot (the r02 figure: the copy, one
                            thread, was what bounded it, not the link)
N>1: the loaded set is replicated, batches are dealt round-robin to the ranks, no data-path collective
(results stay with the rank that computed them, as each GPU would write its own part of the TSV): weak scaling.
"""
from __future__ import annotations

import json
import os
import time

import numpy as np
import torch
import torch.distributed as dist

import distance_amd as da
from tools import synth


def bench_c4(args, rank, world, dev, dev_index, dump=None):
    n_loaded = args.n or 1000
    L = args.len or 5_000_000
    measure = args.measure or "n_high"
    seed = args.seed ^ 4
    B, nb = args.batch, args.batches
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    root = synth.root(seed, L)
    threads = min(len(os.sched_getaffinity(0)), 16)
    loaded = synth.records(seed, root, 0, n_loaded, threads=threads)
    eng = da.Engine(dev_index)
    eng.set_path(args.path)
    eng.upload(0, loaded)
    del loaded
    width = 8
    # this rank's batches of one step: global batch g goes to rank g % world
    mine = [g for g in range(nb * world) if g % world == rank]
    host = torch.empty((len(mine), B, L), dtype=torch.uint8).pin_memory()
    for k, g in enumerate(mine):
        synth.records(seed, root, n_loaded + g * B, B, threads=threads, out=host[k].numpy())
    resident = host.to(dev, non_blocking=False)
    # one result block per batch of a step, as a caller keeps them
    out = torch.empty((len(mine), B, n_loaded), dtype=torch.int64 if measure in da.INT_MEASURES else torch.float64, device=dev)
    pairs_per_step = nb * world * B * n_loaded

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- device-resident: upload_device (pack) + run_rect per batch --------------------------------
    def step_resident():
        for k in range(len(mine)):
            eng.upload_device(1, resident[k].data_ptr(), B, L, L, None, stream.cuda_stream)
            eng.run_rect_device(measure, 1, 0, 0, B, out[k].data_ptr(), out[k].numel() * width, stream=stream.cuda_stream)

    for _ in range(args.warmup):
        step_resident()
    fence()
    k_ms = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step_resident()
        k_ms.append(eng.last_kernel_ms()["pair_ms"])
    fence()
    el_res = time.perf_counter() - t0
    used = eng.last_path()
    dumped = dump(out) if dump is not None else None

    # ---- H2D-inclusive: the overlapped pipeline from page-locked memory ----------------------------
    def step_stream(st, data, copy):
        for k in range(len(mine)):
            if st.in_flight() == st.depth - 1:
                st.pop(copy=False)
            buf, _ = st.buffer()
            if copy:
                buf[:B] = data[k]              # stand-in for "the caller encodes into the buffer": one thread's memcpy
            st.submit(B)
        while st.in_flight():
            st.pop(copy=False)

    h2d = {}
    host_nib = None
    for wire in ("codes", "nibbles") if args.full else ():
        if wire == "nibbles":
            host_nib = [da.engine.Stream.to_nibbles(host[k].numpy()) for k in range(len(mine))]
        data = [host[k].numpy() for k in range(len(mine))] if wire == "codes" else host_nib
        for copy in (False, True):
            with eng.stream(measure, max_records=B, depth=3, nibbles=(wire == "nibbles")) as st:
                # every ring slot holds a real batch before timing starts (the in-place figures re-send what is there)
                for _ in range(max(args.warmup, 1)):
                    step_stream(st, data, True)
                fence()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step_stream(st, data, copy)
                fence()
                el = time.perf_counter() - t0
            h2d[(wire, copy)] = el

    def maxed(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    el_res = maxed(el_res)
    h2d = {k: maxed(v) for k, v in h2d.items()}
    if rank == 0:
        ms = 1e3 * el_res / args.steps
        kernel_ms = float(np.mean(k_ms))
        words = (L + 127) // 128 * 4
        lane_ops = B * n_loaded * words * 5 / (kernel_ms * 1e-3)
        result = {
            "metric": "pairwise comparisons/sec",
            "value": pairs_per_step / (el_res / args.steps),
            "unit": "pairs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic",
            "config": {"workload": f"{n_loaded} x {L} loaded (resident) vs {nb} streamed batches of {B} records per GPU "
                                   f"per step, -m {measure}, streamed-major int64 results in HBM",
                       "name": "C4", "n_loaded": n_loaded, "len": L, "measure": measure, "batch_records": B,
                       "batches_per_step": nb * world, "pairs": pairs_per_step, "path": used,
                       "partition": f"loaded set replicated, batches round-robin over {world} rank(s), no collective",
                       "generator": f"tools/synth (SURVEY 8(d)): xoshiro256**, seed {args.seed:#x} ^ 4"},
            "device_resident": {"pairs_per_s": pairs_per_step / (el_res / args.steps), "ms_per_step": ms,
                                "note": "batches in HBM when timing starts: pack + split-L pair kernel per batch"},
            "roofline": {"bound": "valu", "achieved": lane_ops / 1e12, "peak": 256 * 4 * 32 * 2.4e9 / 1e12,
                         "unit": "Tlane-op/s", "frac": lane_ops / (256 * 4 * 32 * 2.4e9), "kernel": "pair_kernel (split-L)",
                         "kernel_ms": kernel_ms, "traffic": None,
                         "note": "dense n_high: 5 VALU ops per 32 sites per pair; one launch = one batch"},
            "site_compares_per_s": pairs_per_step / (el_res / args.steps) * L,
        }
        if dumped:
            result["dump_outputs"] = dumped
        if args.full:
            result["h2d_inclusive"] = {
                **{f"{wire}{'_with_host_copy' if copy else ''}": {
                    "pairs_per_s": pairs_per_step / (h2d[(wire, copy)] / args.steps),
                    "ms_per_step": 1e3 * h2d[(wire, copy)] / args.steps,
                    "link_GBps": nb * B * (L if wire == "codes" else (L + 1) // 2) / (h2d[(wire, copy)] / args.steps) / 1e9}
                   for wire in ("codes", "nibbles") for copy in (False, True)},
                "note": "page-locked host batches through dst_stream_* (depth 3): H2D, pack, compare, D2H overlapped; never "
                        "reported as `value`.  codes: Paradis bytes; nibbles: DST_WIRE_NIBBLES (half the bytes).  "
                        "*_with_host_copy adds a one-thread memcpy of every batch into its ring slot, the stand-in for a parser "
                        "that does not write into the slot directly"}
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()
