"""The thread-rank communicator of the shared-upload tests: the ranks are THREADS of this process, each with its own
context on GPU 0, joined by a communicator over a custom transport (dst_comm_create_custom): an all-gather through host
memory behind a threading.Barrier.  That runs every line of dst_upload_shared except RCCL's ncclAllGather call itself."""
import ctypes as C
import threading

import numpy as np

import distance_amd as da


class ThreadRanks:
    """world threads, one context each, an all-gather through host memory"""

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.blocks = [None] * world
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    def allgather(self, rank):
        def fn(d_send, d_recv, nbytes, stream):
            assert self.hip.hipStreamSynchronize(stream) == 0
            host = np.empty(nbytes, np.uint8)
            assert self.hip.hipMemcpy(host.ctypes.data, d_send, nbytes, 2) == 0
            self.blocks[rank] = host
            self.barrier.wait()
            everything = np.concatenate(self.blocks)
            assert self.hip.hipMemcpy(d_recv, everything.ctypes.data, everything.nbytes, 1) == 0
            self.barrier.wait()           # nobody overwrites its block before everybody has read it
        return fn

    def run(self, body):
        """body(rank, eng, comm) on every rank; returns the list of results (exceptions re-raised)"""
        out, err = [None] * self.world, [None] * self.world

        def work(rank):
            try:
                with da.Engine(0) as eng, da.Comm.custom(eng, rank, self.world, self.allgather(rank)) as comm:
                    out[rank] = body(rank, eng, comm)
            except BaseException as e:   # noqa: BLE001 - reported below
                err[rank] = e
                self.barrier.abort()

        th = [threading.Thread(target=work, args=(r,)) for r in range(self.world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for e in err:
            if e is not None and not isinstance(e, threading.BrokenBarrierError):
                raise e
        for e in err:
            if e is not None:
                raise e
        return out


def single_engine(codes, measures, tallies=False):
    with da.Engine(0) as eng:
        eng.set_path("dense")
        eng.upload(0, codes)
        return {m: eng.run_square(m, tallies=tallies) for m in measures}
