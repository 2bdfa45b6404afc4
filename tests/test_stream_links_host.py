"""CPU: the links-stream additions to the C ABI without a GPU — exported, declared, ABI version unchanged, and the
calls refuse a NULL context or stream."""
import ctypes as C

import distance_amd as da

NEW = ("dst_stream_open_links", "dst_stream_links_batch", "dst_stream_links_stats")
ERR_ARG = 1


def test_symbols_are_declared_and_exported():
    lib = da.load()
    declared = da.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_abi_version_is_unchanged():
    assert da.load().dst_abi_version() == 3


def test_null_context_and_stream_are_argument_errors():
    lib = da.load()
    h = C.c_void_p(1)
    assert lib.dst_stream_open_links(None, 2, 5.0, 1, 0, 8, 3, 0, C.byref(h)) == ERR_ARG
    assert lib.dst_stream_open_links(None, 2, 5.0, 1, 0, 8, 3, 0, None) == ERR_ARG
    n, total = C.c_uint64(7), C.c_uint64(7)
    sp, lp, vp, tp = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.dst_stream_links_batch(None, 0, C.byref(n), C.byref(total), C.byref(sp), C.byref(lp), C.byref(vp),
                                      C.byref(tp)) == ERR_ARG
    assert lib.dst_stream_links_batch(None, 0, None, None, None, None, None, None) == ERR_ARG
    assert lib.dst_stream_links_stats(None, C.byref(n), C.byref(total)) == ERR_ARG
    assert lib.dst_stream_links_stats(None, None, None) == ERR_ARG


def test_the_default_window_is_the_headers():
    text = open(da._lib.HEADER_PATH).read()
    assert "#define DST_STREAM_LINKS_WINDOW (1u << 20)" in text
    assert da._lib.STREAM_LINKS_WINDOW == 1 << 20 <= da._lib.LINKS_CHUNK


def test_python_surface():
    assert hasattr(da.Engine, "links_stream") and issubclass(da.LinksStream, da.engine.Stream)
    for name in ("pop", "links_batch", "stats", "buffer", "submit", "push", "in_flight", "to_nibbles"):
        assert hasattr(da.LinksStream, name), name
