"""The designed set of the window-closest stream tests (dst_stream_open_window_closest, --window-closest): a loaded set of
up to nine records and 300 streamed records of 300 sites, the windows, the batch cuts, and the numpy restatement of the
definition.  No GPU, no distance_amd."""
import numpy as np

from helpers import random_alignment
from window_nearest_reference import keys, nearest, oracle_payloads

L = 300               # two full 128-site chunks and a cut third
N_STREAMED = 300
N_CODE = 240          # 'N'
LOADED_SIZES = (1, 8, 9)   # the sweep's row tile holds eight
# in this order: the whole width; a window that cuts two chunks; one exact chunk; one site; an empty one; the last site; a
# repeat; the first chunk
WINDOWS = np.array([(0, 300), (5, 133), (128, 256), (130, 131), (7, 7), (299, 300), (5, 133), (0, 128)], np.uint64)
# the stream cut into batches, max_records = 257
MAX_RECORDS = 257
CUTS = ([257, 43], [64, 65, 171], [1] * 5 + [256, 39], [255, 45])
TIE_CUT = [64, 65, 171]
# exact copies of loaded record 0 among the streamed records: four candidates at key 0 for every window of record 0, the
# third in batch 1 and the fourth in batch 2 of TIE_CUT (batches [0, 64), [64, 129), [129, 300))
COPIES_OF_LOADED_0 = (5, 70, 100, 200)
# exact duplicates of one another (not of a loaded record), in different batches of every cut above
DUPLICATES = ((17, 150), (63, 64), (128, 129), (2, 299), (254, 255), (256, 257))
ALL_N = 250           # a streamed record that is N at every site: raw NaN in every window, after every number; n: 0


def loaded_set() -> np.ndarray:
    return random_alignment(9, L, seed=811, p_ambig=0.04, p_gap=0.03, divergence=0.08)


def streamed_set() -> np.ndarray:
    loaded = loaded_set()
    s = random_alignment(N_STREAMED, L, seed=812, p_ambig=0.04, p_gap=0.03, divergence=0.08, root=loaded[0])
    for at in COPIES_OF_LOADED_0:
        s[at] = loaded[0]
    for a, b in DUPLICATES:
        s[b] = s[a]
    s[ALL_N] = N_CODE
    return np.ascontiguousarray(s)


def batches(cut):
    """[(first ordinal, end)] of a cut"""
    out, at = [], 0
    for n in cut:
        out.append((at, at + n))
        at += n
    assert at == N_STREAMED
    return out


def batch_of(cut, ordinal: int) -> int:
    return next(b for b, (lo, hi) in enumerate(batches(cut)) if lo <= ordinal < hi)


def reference(measure: str, loaded: np.ndarray, streamed: np.ndarray, k: int, windows=WINDOWS):
    """(index[n_loaded, n_windows, k_used], payloads[n_windows, n_loaded, n_streamed]) of n / n_high / raw: the definition
    through the oracle on the cut columns, ascending (key, ordinal)"""
    payloads = oracle_payloads(measure, loaded, streamed, windows)
    return nearest(payloads, k), payloads


def sorted_keys(payloads: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(order, keys in that order), both [n_windows, n_loaded, n_streamed]: every candidate, ascending (key, ordinal)"""
    kk = keys(payloads)
    order = np.argsort(kk, axis=2, kind="stable")
    return order, np.take_along_axis(kk, order, axis=2)
