"""The PGX convolutional network (envpool_amd/csrc/pgx_conv.hip.h, DESIGN.md "PGX convolutional network") restated in
numpy, independently of the header: a 3x3 cross-correlation as nine shifted int64 matrix products over a zero-padded
board (the contract's int32 bound is asserted), `rs`, the clamps and `outputs` of pgx_net_util; the nets' recipe."""
import numpy as np

from pgx_net_util import outputs, rs

CASES = [(3, 3, 2, 9, 32, 1, 4), (6, 7, 2, 7, 64, 1, 4), (8, 8, 2, 65, 64, 2, 8), (11, 11, 4, 122, 32, 1, 4),
         (8, 8, 2, 65, 128, 1, 2), (8, 8, 2, 65, 256, 1, 1)]  # H, W, C, A, D, L, P
SEEDS = {case: 0 for case in CASES}
SEEDS[(8, 8, 2, 65, 256, 1, 1)] = 1  # (seed 0 has a dead reduce plane)
LOWERED = (8, 8, 2, 65, 64, 2, 8)  # the extra case: every shift lowered by 2, which makes 127 common
ALL = [case + (0,) for case in CASES] + [LOWERED + (-2,)]
ROWS = (1, 31, 33, 100)


def random_layers(h, w, c, a, d, blocks, p, seed, shift_delta=0):
    """The issue's recipe: PCG64(seed); layer by layer in blob order, weights uniform in [-127, 127] before biases
    uniform in [-1024, 1024]; shifts max(0, . + shift_delta) of round(log2(73 sqrt(9 C / 4) / 32)) for the stem,
    round(log2(73 sqrt(9 D) 40 / 32)) for the block layers, round(log2(73 sqrt(D) 40 / 32)) for the reduce layer."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shifts = ([np.log2(73.0 * np.sqrt(9 * c / 4.0) / 32.0)] + [np.log2(73.0 * np.sqrt(9 * d) * 40.0 / 32.0)] * (2 * blocks)
              + [np.log2(73.0 * np.sqrt(d) * 40.0 / 32.0)])
    layers = []
    for i, shape in enumerate([(d, 3, 3, c)] + [(d, 3, 3, d)] * (2 * blocks) + [(p, d), (a + 1, h * w * p)]):
        wt = rng.integers(-127, 128, size=shape).astype(np.int8)
        b = rng.integers(-1024, 1025, size=shape[0]).astype(np.int32)
        layers.append((wt, b, 0 if i == 2 * blocks + 2 else max(0, int(round(shifts[i])) + shift_delta)))
    return layers


def scales(h, w, p):
    spread = 73.0 * np.sqrt(h * w * p) * 40.0
    return np.float32(4.0 / spread), np.float32(1.0 / spread)


def make_blob(h, w, c, a, d, blocks, p, layers, scale_p, scale_v, magic=0x43584750, version=1, tail=0):
    """The blob by hand (no envpool_amd code): header, then per layer matrix, padding, bias, shift."""
    parts = [np.array([magic, version, h, w, c, a, d, blocks, p], "<i4").tobytes(),
             np.array([scale_p, scale_v], "<f4").tobytes(), np.array([tail], "<i4").tobytes()]
    for wt, b, shift in layers:
        raw = np.ascontiguousarray(wt, np.int8).tobytes()
        parts += [raw, b"\0" * (-len(raw) % 4), np.ascontiguousarray(b, "<i4").tobytes(),
                  np.array([shift], "<i4").tobytes()]
    return np.frombuffer(b"".join(parts), np.uint8).copy()


def conv(wt, b, x):
    """x int64 [rows, H, W, K], wt [N, 3, 3, K] -> [rows, H, W, N]: zero padding, cross-correlation."""
    rows, h, w, _ = x.shape
    pad = np.zeros((rows, h + 2, w + 2, x.shape[3]), np.int64)
    pad[:, 1:-1, 1:-1] = x
    z = np.zeros((rows, h, w, wt.shape[0]), np.int64) + b.astype(np.int64)
    for dy in range(3):
        for dx in range(3):
            z += pad[:, dy:dy + h, dx:dx + w] @ wt[:, dy, dx].astype(np.int64).T
    assert np.abs(z).max() < 2 ** 31 - 2 ** 24  # the contract's bound, rounding term included
    return z


def integers(layers, blocks, obs_shape, obs):
    """(p int64 [rows, A + 1], the hidden activations before their clamps as a list of int64 arrays)."""
    x = np.asarray(obs).reshape((-1,) + tuple(obs_shape)).astype(np.int64)
    pre = [rs(conv(*layers[0][:2], x), layers[0][2])]
    h = np.clip(pre[-1], 0, 127)
    for l in range(blocks):
        w1, b1, s1 = layers[1 + 2 * l]
        w2, b2, s2 = layers[2 + 2 * l]
        pre.append(rs(conv(w1, b1, h), s1))
        t = np.clip(pre[-1], 0, 127)
        pre.append(rs(conv(w2, b2, t), s2) + h)
        h = np.clip(pre[-1], 0, 127)
    wr, br, sr = layers[2 * blocks + 1]
    pre.append(rs(h @ wr.astype(np.int64).T + br.astype(np.int64), sr))
    g = np.clip(pre[-1], 0, 127).reshape(len(x), -1)  # (y, x, q)
    wh, bh, _ = layers[2 * blocks + 2]
    p = g @ wh.astype(np.int64).T + bh.astype(np.int64)
    assert np.abs(p).max() < 2 ** 31 - 2 ** 24
    return p, pre


def restate(layers, blocks, obs_shape, scale_p, scale_v, obs, mask, status, priors):
    status = np.asarray(status).reshape(-1)
    mask = np.asarray(mask).reshape(len(status), -1).astype(np.uint8)
    p, _ = integers(layers, blocks, obs_shape, np.asarray(obs).astype(np.uint8))
    return outputs(p, mask, status, scale_p, scale_v, priors)


def check_spread(layers, blocks, obs_shape, obs, lowered=False):
    """The issue's input condition (a failure is a mistake of the test): both clamps are hit and a quarter of the hidden
    pre-activations lies strictly inside; for the lowered case both clamps are hit and a quarter sits at 127."""
    _, pre = integers(layers, blocks, obs_shape, obs)
    z = np.concatenate([x.reshape(-1) for x in pre])
    assert (z <= 0).any() and (z >= 127).any(), "both clamps must be hit"
    share = (z >= 127).mean() if lowered else ((z > 0) & (z < 127)).mean()
    assert share >= 0.25, f"only {share:.2f} of the activations " + ("are at 127" if lowered else "lie strictly inside")
