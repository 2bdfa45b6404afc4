"""CPU: the closest-stream additions to the C ABI without a GPU — exported, declared, ABI version unchanged, and the
calls refuse a NULL stream."""
import ctypes as C

import distance_amd as da

NEW = ("dst_stream_open_closest", "dst_stream_closest_next_index", "dst_stream_closest_result", "dst_stream_closest_batch")
ERR_ARG = 1


def test_symbols_are_declared_and_exported():
    lib = da.load()
    declared = da.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_abi_version_is_unchanged():
    assert da.load().dst_abi_version() == 3


def test_null_stream_is_an_argument_error():
    lib = da.load()
    ku, p = C.c_uint32(7), C.c_void_p()
    index = (C.c_uint32 * 4)()
    assert lib.dst_stream_closest_next_index(None, 5) == ERR_ARG
    assert lib.dst_stream_closest_result(None, index, None, None, 4, C.byref(ku)) == ERR_ARG
    assert lib.dst_stream_closest_batch(None, C.byref(p), None, None, C.byref(ku)) == ERR_ARG
    h = C.c_void_p(1)
    assert lib.dst_stream_open_closest(None, 2, 5, 0, 8, 3, 0, C.byref(h)) == ERR_ARG
    assert lib.dst_stream_open_closest(None, 2, 5, 0, 8, 3, 0, None) == ERR_ARG


def test_python_surface():
    assert hasattr(da.Engine, "closest_stream") and issubclass(da.ClosestStream, da.engine.Stream)
    for name in ("pop", "result", "next_index", "buffer", "submit", "push", "to_nibbles"):
        assert hasattr(da.ClosestStream, name), name
