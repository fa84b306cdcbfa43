"""numpy restatement of the epoch permutations of train_uci.py -device_batches (gnf_shuffle_keys, include/gnf_hip.h), on
toy_ref.py's philox4x32_10.  Imported by tests/test_uci_batches_host.py and tests/test_gpu_tab_batch.py."""
import numpy as np

from toy_ref import philox4x32_10

_LO = np.uint64(0xffffffff)


def shuffle_keys(seed, offset, n):
    """int64 keys [n]: keys[i] = ((r[i & 3] >> 1) << 32) | i, r the Philox words of counter (lo32(i >> 2), 0, lo32(offset),
    hi32(offset)) under key (lo32(seed), hi32(seed))"""
    i = np.arange(n, dtype=np.uint64)
    seed, offset = np.uint64(seed), np.uint64(offset)
    words = philox4x32_10(i >> np.uint64(2), 0, offset & _LO, offset >> np.uint64(32), seed & _LO, seed >> np.uint64(32))
    r = np.choose((i & np.uint64(3)).astype(np.int64), [np.broadcast_to(w, i.shape) for w in words]) if n else i
    keys = ((r >> np.uint64(1)) << np.uint64(32)) | i
    assert n == 0 or int(keys.max()) < 1 << 63                       # 31 random bits: non-negative as int64
    return keys.astype(np.int64)


def permutation(seed, offset, n):
    """int32 [n]: the low words of the sorted keys"""
    return (np.sort(shuffle_keys(seed, offset, n)) & np.int64(0xffffffff)).astype(np.int32)
