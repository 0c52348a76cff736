"""The PGX built-in network (envpool_amd/csrc/pgx_net.hip.h, DESIGN.md "PGX built-in network") restated in numpy,
independently of the header: int64 matrix products (exact: nothing comes near 2^63, and the contract's own bound keeps
every value inside int32, which `restate` asserts), the rounding shift, the clamps, and the float32 outputs with the
Gumbel kernels' exponential (pgx_gumbel_util.exp_).  Plus the recipe of the tests' random nets and inputs, and the
blob written by hand."""
import numpy as np

from pgx_gumbel_util import exp_

F32 = np.float32
CASES = [(18, 9, 32, 0), (84, 7, 64, 1), (128, 65, 128, 2), (484, 122, 96, 2), (128, 65, 512, 1)]  # F, A, D, L
ROWS = (1, 31, 33, 100)
# The seed of each case's net: the first for which the 100-row input meets check_spread -- a property of this
# restatement's own numbers (trunks of 32 neurons see few biases; Hex's upper clamp is rare), found without the code
# under test.
SEEDS = {(18, 9, 32, 0): 0, (84, 7, 64, 1): 0, (128, 65, 128, 2): 0, (484, 122, 96, 2): 5, (128, 65, 512, 1): 0}
LOWERED = (128, 65, 128, 2)  # the extra case: every shift lowered by 2, which makes 127 common


def random_layers(f, a, d, blocks, seed, shift_delta=0):
    """The issue's recipe: PCG64(seed); weights uniform in [-127, 127], biases uniform in [-1024, 1024], input shift
    round(log2(73 sqrt(F / 4) / 32)), hidden shifts round(log2(73 sqrt(D) 40 / 32)); `shift_delta` is added to each."""
    rng = np.random.Generator(np.random.PCG64(seed))
    s_in = int(round(np.log2(73.0 * np.sqrt(f / 4.0) / 32.0)))
    s_hid = int(round(np.log2(73.0 * np.sqrt(d) * 40.0 / 32.0)))
    layers = []
    for i in range(2 * blocks + 2):
        head = i == 2 * blocks + 1
        n, k = (a + 1 if head else d), (f if i == 0 else d)
        w = rng.integers(-127, 128, size=(n, k)).astype(np.int8)
        b = rng.integers(-1024, 1025, size=n).astype(np.int32)
        layers.append((w, b, 0 if head else max(0, (s_in if i == 0 else s_hid) + shift_delta)))
    return layers


def scales(d):
    """(scale_p, scale_v) that put the logits at a few units and the values around +-1, as float32."""
    spread = 73.0 * np.sqrt(d) * 40.0
    return F32(4.0 / spread), F32(1.0 / spread)


def random_rows(f, a, rows, seed):
    """Inputs of density 0.25, masks of density 0.5 with at least one legal action (every fifth row exactly one), a mix
    of statuses 0 / 1 / 2 (mostly 0; row 0 is 0)."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    obs = (rng.random((rows, f)) < 0.25).astype(np.uint8)
    mask = (rng.random((rows, a)) < 0.5).astype(np.uint8)
    one = rng.integers(0, a, size=rows)
    mask[np.arange(rows), one] = 1
    single = np.arange(rows) % 5 == 4
    mask[single] = 0
    mask[single, one[single]] = 1
    status = rng.choice(np.array([0, 0, 0, 0, 1, 2], np.uint8), size=rows)
    status[0] = 0
    return obs, mask, status


def make_blob(f, a, d, blocks, layers, scale_p, scale_v, magic=0x4E584750, version=1):
    """The blob by hand (no envpool_amd code): header, then per layer matrix, padding, bias, shift."""
    parts = [np.array([magic, version, f, a, d, blocks], "<i4").tobytes(),
             np.array([scale_p, scale_v], "<f4").tobytes()]
    for w, b, shift in layers:
        raw = np.ascontiguousarray(w, np.int8).tobytes()
        parts += [raw, b"\0" * (-len(raw) % 4), np.ascontiguousarray(b, "<i4").tobytes(),
                  np.array([shift], "<i4").tobytes()]
    return np.frombuffer(b"".join(parts), np.uint8).copy()


def rs(x, s):
    return (x + ((1 << (s - 1)) if s else 0)) >> s  # (numpy's >> on signed integers is arithmetic)


def integers(layers, blocks, obs):
    """(p int64 [rows, A + 1], the hidden activations before their clamps as a list of int64 arrays)."""
    def lin(i, x):
        w, b, _ = layers[i]
        z = x @ w.astype(np.int64).T + b.astype(np.int64)
        assert np.abs(z).max() < 2 ** 31 - 2 ** 24  # the contract's bound, rounding term included
        return z

    pre = []
    x = obs.astype(np.int64)
    z = rs(lin(0, x), layers[0][2])
    pre.append(z)
    h = np.clip(z, 0, 127)
    for l in range(blocks):
        z = rs(lin(1 + 2 * l, h), layers[1 + 2 * l][2])
        pre.append(z)
        t = np.clip(z, 0, 127)
        z = rs(lin(2 + 2 * l, t), layers[2 + 2 * l][2]) + h
        pre.append(z)
        h = np.clip(z, 0, 127)
    return lin(2 * blocks + 1, h), pre


def outputs(p, mask, status, scale_p, scale_v, priors):
    """The float32 outputs of the contract from the head's integers."""
    rows, a = mask.shape
    logits = p[:, :a].astype(np.int32).astype(F32) * F32(scale_p)
    value = np.clip(p[:, a].astype(np.int32).astype(F32) * F32(scale_v), F32(-1), F32(1)).astype(F32)
    assert logits.dtype == F32 and value.dtype == F32
    policy = logits.copy()
    if priors:
        policy = np.zeros((rows, a), F32)
        for r in range(rows):
            legal = np.flatnonzero(mask[r])
            if len(legal) == 0:
                continue
            e = exp_(logits[r, legal] - logits[r, legal].max())
            total = F32(0)
            for x in e:  # ascending action order
                total = F32(total + x)
            policy[r, legal] = e / total
    idle = status != 0
    policy[idle] = 0
    value[idle] = 0
    return policy, value


def restate(layers, blocks, scale_p, scale_v, obs, mask, status, priors):
    obs = np.asarray(obs).reshape(len(np.asarray(status).reshape(-1)), -1).astype(np.uint8)
    mask = np.asarray(mask).reshape(len(obs), -1).astype(np.uint8)
    p, _ = integers(layers, blocks, obs)
    return outputs(p, mask, np.asarray(status).reshape(-1), scale_p, scale_v, priors)


def check_spread(layers, blocks, obs, lowered=False):
    """The two conditions a test input must meet (a failure is a mistake of the test): over the hidden layers both
    clamps are hit, and at least a quarter of the activations lie strictly inside.  The case with lowered shifts is
    there for the upper clamp -- with shifts 2 lower a fifth lies inside, whatever the seed -- so it must hit both
    clamps and have 127 in at least a quarter of the activations."""
    _, pre = integers(layers, blocks, obs)
    z = np.concatenate([x.reshape(-1) for x in pre])
    assert (z <= 0).any() and (z >= 127).any(), "both clamps must be hit"
    if lowered:
        assert (z >= 127).mean() >= 0.25, f"only {(z >= 127).mean():.2f} of the activations are at the upper clamp"
        return
    inside = ((z > 0) & (z < 127)).mean()
    assert inside >= 0.25, f"only {inside:.2f} of the activations lie strictly inside"


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)
