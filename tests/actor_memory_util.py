"""The memory cell's contract (envpool_amd/csrc/actor_memory.hip.h) restated in numpy, independently of the header, in
int64: nothing here can wrap, so equality with the int32 builds also says that those did not."""
import numpy as np


def rs(x, s):
    return (x + ((1 << (s - 1)) if s else 0)) >> s


def cell(layers, x, h):
    """h' uint8 [rows, M] of feature rows x [rows, F] and states h [rows, M]; layers = ((Wz, bz, sz), (Wn, bn, sn))."""
    (wz, bz, sz), (wn, bn, sn) = layers
    h = np.asarray(h, np.int64)
    v = np.concatenate([np.asarray(x, np.int64), h], axis=1)
    z = np.clip(64 + rs(v @ wz.astype(np.int64).T + bz.astype(np.int64), sz), 0, 128)
    n = np.clip(rs(v @ wn.astype(np.int64).T + bn.astype(np.int64), sn), 0, 127)
    out = (z * h + (128 - z) * n + 64) >> 7
    assert out.min() >= 0 and out.max() <= 127
    return out.astype(np.uint8)
