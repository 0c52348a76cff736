"""Plain NumPy reference of the Atari post-process (AtariEnv::PushStack, atari_env.h:308-346) with
everything the HIP kernel does around the resize: the colour palette, one or three planes per
stacked frame and the four per-row flags of include/envpool_amd.h.  TEST INFRASTRUCTURE.

The stack is held as `[n, S, C, h, w]` in LOGICAL order, oldest to newest (no ring).  Only the
single-plane resize is not NumPy: it is `orc_resize_area_u8` / `orc_resize_linear_u8` of
oracle/atari/atari_post.c, called as they are.
"""
import ctypes

import numpy as np

from oracle.orc import PORT_LIB

_lib = None


def _resize_fn(linear):
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(PORT_LIB)
        for fn in (_lib.orc_resize_area_u8, _lib.orc_resize_linear_u8):
            fn.restype = None
            fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                           ctypes.c_int]
    return _lib.orc_resize_linear_u8 if linear else _lib.orc_resize_area_u8


def resize(plane, oh, ow, linear=False):
    """cv::resize of one 8UC1 plane as the oracle restates it."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    out = np.empty((oh, ow), np.uint8)
    _resize_fn(linear)(plane.ctypes.data, plane.shape[0], plane.shape[1], out.ctypes.data, oh, ow)
    return out


class RefPost:
    """`palette`: None (frames are pixel values; gray only), [256] (gray) or [3, 256] (RGB).
    `lookup_first=False` is the WRONG order (max of the indices, then the palette): it exists so
    that a test can show that its input tells the two orders apart."""

    def __init__(self, n, s=4, oh=84, ow=84, raw=(210, 160), linear=False, gray=True, palette=None,
                 lookup_first=True):
        assert gray or palette is not None
        self.n, self.s, self.oh, self.ow, self.raw, self.linear = n, s, oh, ow, tuple(raw), linear
        self.c = 1 if gray else 3
        self.lut = None if palette is None else np.asarray(palette, np.uint8).reshape(self.c, 256)
        self.lookup_first = lookup_first
        self.stack = np.zeros((n, s, self.c, oh, ow), np.uint8)
        # position of the kernel's ring head: pushes since the last fill, modulo S
        self.pushes = np.zeros(n, np.int64)

    def heads(self):
        return self.pushes % self.s

    def _frame(self, f0, f1, flag):
        """The new stacked frame [C, h, w] of one row."""
        out = np.empty((self.c, self.oh, self.ow), np.uint8)
        for c in range(self.c):
            if self.lut is None:
                pooled = np.maximum(f0, f1) if flag == 0 else f0
            elif flag != 0:
                pooled = self.lut[c][f0]
            elif self.lookup_first:
                pooled = np.maximum(self.lut[c][f0], self.lut[c][f1])
            else:
                pooled = self.lut[c][np.maximum(f0, f1)]
            out[c] = resize(pooled, self.oh, self.ow, self.linear)
        return out

    def push(self, frames, ids=None, mask=None):
        k = frames.shape[0]
        assert frames.shape == (k, 2, *self.raw) and frames.dtype == np.uint8
        ids = np.arange(k) if ids is None else ids
        obs = np.empty((k, self.s * self.c, self.oh, self.ow), np.uint8)
        for i in range(k):
            e, flag = int(ids[i]), 0 if mask is None else int(mask[i])
            assert flag in (0, 1, 2, 4), flag
            st = self.stack[e]
            new = st[-1].copy() if flag == 4 else self._frame(frames[i, 0], frames[i, 1], flag)
            if flag == 1:  # reset: the frame shows in every slot
                st[:] = new
                self.pushes[e] = 0
            else:  # 0, 2, 4: drop the oldest, append
                st[:-1] = st[1:].copy()
                st[-1] = new
                self.pushes[e] += 1
            obs[i] = st.reshape(self.s * self.c, self.oh, self.ow)  # [slot][plane], atari_env.h:320-335
        return obs


def random_palette(rng, gray):
    """A non-monotone palette that still takes every value: one random permutation per plane."""
    pal = np.stack([rng.permutation(256) for _ in range(1 if gray else 3)]).astype(np.uint8)
    return pal[0] if gray else pal


def sparse_frames(rng, k, raw=(210, 160)):
    """Console-like frames: one background value per frame and a few rectangles."""
    h, w = raw
    f = np.empty((k, 2, h, w), np.uint8)
    for i in range(k):
        for j in range(2):
            f[i, j] = rng.integers(0, 256)
            for _ in range(8):
                y, x = rng.integers(0, h - 4), rng.integers(0, w - 4)
                f[i, j, y:y + rng.integers(2, 24), x:x + rng.integers(1, 12)] = rng.integers(0, 256)
    return f


def scripted_sequence(rng, n, raw=(210, 160)):
    """At least 12 pushes `(frames, ids, mask)` over a pool of n >= 8 envs that between them hold:
    an all-reset push, flag-0 pushes, pushes whose rows mix 0 / 1 / 2 / 4, flag 4 directly after
    flag 1, two flag-4 pushes in a row, and partial pushes with shuffled ids -- the first of them
    without flag 1, so that afterwards the ring heads differ between envs."""
    assert n >= 8
    ids = np.arange(n, dtype=np.int32)

    def noise(k):
        return rng.integers(0, 256, (k, 2, *raw), dtype=np.uint8)

    def full(flags):
        return np.resize(np.asarray(flags, np.uint8), n)

    k0 = n - 3
    seq = [
        (noise(n), ids, full([1])),                    # 0  all reset
        (sparse_frames(rng, n, raw), ids, None),       # 1  flag 0, no mask at all
        (noise(n), ids, full([0])),                    # 2  flag 0, mask of zeros
        (sparse_frames(rng, n, raw), ids, full([0, 1, 2, 4])),  # 3  every flag in one push
        (noise(n), ids, full([4])),                    # 4  flag 4: directly after flag 1 on envs 1, 5, ...
        (noise(n), ids, full([4])),                    # 5  flag 4 again
        (noise(n), ids, None),                         # 6
        (sparse_frames(rng, k0, raw), rng.permutation(n)[:k0].astype(np.int32),
         np.resize(np.asarray([0, 2, 4], np.uint8), k0)),       # 7  partial, no fill: heads diverge
        (noise(n), ids, None),                         # 8  flag 0 on diverged heads
        (noise(k0), rng.permutation(n)[:k0].astype(np.int32),
         np.resize(np.asarray([4, 1, 0, 2], np.uint8), k0)),    # 9  partial, every flag
        (sparse_frames(rng, n, raw), ids, rng.permutation(full([2, 4, 1, 0]))),  # 10
        (noise(n), ids, None),                         # 11
        (sparse_frames(rng, n, raw), ids, full([2])),  # 12 single frames pushed like steps
        (noise(n), ids, None),                         # 13
    ]
    return seq, 7  # the index of the push after which the heads must differ
