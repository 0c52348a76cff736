"""Snapshot, restore and fork on the device: a restored env continues bit for bit -- every key of every row, resets and
their draws included -- through the host blob and through the device blob, into the same pool, into another pool,
with a frame stack, from an async pool, from the last rows of a big pool and across shards; what a pool refuses.

num_envs = 40 is no multiple of 16 or 64 (the last generator tile group and the last wave are partial); the subset
IDS is out of order and straddles a 16-env boundary.  Episodes are 5 to 7 steps long, so that every run of 12 steps
holds at least one reset -- and hence generator draws -- of every env."""
import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core.device_pool import DevicePool

pytestmark = pytest.mark.gpu

N = 40
IDS = np.array([39, 0, 17, 16, 15, 3], dtype=np.int32)
IDS2 = np.array([1, 38, 5, 20, 21, 9], dtype=np.int32)
STEPS = 12
ID_KEYS = ("info:env_id", "info:players.env_id")

# one registered id per step kernel -> max_episode_steps
TASKS = {
    "CartPole-v1": 6, "Pendulum-v1": 5, "Blackjack-v1": 6, "FrozenLake8x8-v1": 7, "HalfCheetah-v4": 6,
    "Hopper-v4/planar_layout=0": 6, "Hopper-v4/planar_layout=1": 6, "Ant-v4": 6, "InvertedDoublePendulum-v4": 6,
    "Reacher-v4": 6, "Pusher-v4": 6, "Humanoid-v4": 6, "MiniGrid-Dynamic-Obstacles-6x6-v0": 6,
    "MiniGrid-DoorKey-5x5-v0": 7, "Game2048-v1": 6, "Snake-v1": 6, "Minesweeper-v0": 5, "Othello-v1": 7, "Hex-v1": 7,
}
# Game2048 only reports `trunc` against max_episode_steps and plays on (a random player's game lasts far longer than a
# test): it has no reset inside a window, but every one of its steps draws (the spawned tile)
DRAWS_EVERY_STEP = {"Game2048-v1"}


class Handle:
    """A pool under test: the gymnasium env (whose snapshot / restore / fork are the calls under test) and its
    DevicePool (through which every state key of every row is recorded).  A case with an engine key
    ("Hopper-v4/planar_layout=1"), or with `engine_keys`, has no env: engine keys do not pass through `make`, the
    DevicePool is the handle."""

    def __init__(self, case, seed, n=N, engine_keys=None, **kw):
        from mj_util import GYM_VARIANTS, native_variant

        task, _, key = case.partition("/")
        if "max_episode_steps" not in kw:
            kw["max_episode_steps"] = TASKS[case] if case in TASKS else TASKS[task]
        self.space = envpool.make_spec(task).action_space
        keys = dict([key.split("=")] if key else [], **(engine_keys or {}))
        keys = {name: float(value) for name, value in keys.items()}
        if keys:
            self.env = None
            if task in GYM_VARIANTS:
                family, _, params = native_variant(task)
                self.pool = DevicePool(family, n, seed=seed, max_episode_steps=kw.pop("max_episode_steps"),
                                       params={**params, **keys, **kw})
            else:
                from hip_util import registered_pool

                self.pool = registered_pool(task, n, seed, keys, **kw)
            self.api = self.pool
        else:
            self.env = envpool.make(task, env_type="gymnasium", num_envs=n, seed=seed, **kw)
            self.pool = self.env.device_pool
            self.api = self.env
        self.n = n
        self.ids = np.arange(self.pool.env_id_offset, self.pool.env_id_offset + n, dtype=np.int32)

    def actions(self, rng, n=None):
        n = self.n if n is None else n
        sp = self.space
        if hasattr(sp, "n"):
            return rng.integers(0, sp.n, n).astype(self.pool.action_dtype)
        if np.issubdtype(sp.dtype, np.integer):
            return rng.integers(sp.low, sp.high + 1, (n, *sp.shape)).astype(self.pool.action_dtype)
        return rng.uniform(sp.low, sp.high, (n, *sp.shape)).astype(self.pool.action_dtype)

    def reset(self):
        self.pool.reset(self.ids)
        return self.rows()

    def step(self, act, ids=None):
        self.pool.send(self.ids if ids is None else ids, act)
        return self.rows()

    def rows(self):
        """Every state key of the batch, one row per env ([rows, -1]: a per-player key's player rows side by side)."""
        d = self.pool.recv_dict()
        rows = len(d["info:env_id"])
        return {k: np.array(v).reshape(rows, -1) for k, v in d.items()}

    def run(self, acts):
        return [self.step(a) for a in acts]

    def close(self):
        (self.env or self.pool).close()


def same_bits(a, b, tag):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (tag, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.argwhere(a.view(np.uint8) != b.view(np.uint8))
    assert bad.size == 0, (tag, bad[:4].tolist())


def same_rows(got, want, tag, rows_got=None, rows_want=None, skip=()):
    """Lists of per-step row dicts: every key (but `skip`) of the chosen rows, bit for bit."""
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), tag
        for k in g:
            if k in skip:
                continue
            same_bits(g[k] if rows_got is None else g[k][rows_got], w[k] if rows_want is None else w[k][rows_want],
                      (tag, t, k))


def warm_up(h, rng, steps=STEPS):
    h.reset()
    for _ in range(steps):
        h.step(h.actions(rng))


def continuation(h, tag):
    """Test 1: step, snapshot, step on, restore, step the same actions again -- through the host blob and through
    the device blob, which must be the same bytes."""
    import torch

    from envpool_amd import torch_interop as ti

    rng = np.random.default_rng(3)
    warm_up(h, rng)
    blob = h.api.snapshot()
    assert blob.dtype == np.uint8 and blob.nbytes == h.pool.snapshot_bytes(h.n)
    dblob = ti.snapshot_device(h.pool)
    assert dblob.dtype == torch.uint8 and dblob.is_cuda
    same_bits(dblob.cpu().numpy(), blob, (tag, "device blob == host blob"))
    acts = [h.actions(rng) for _ in range(STEPS)]
    first = h.run(acts)
    assert tag in DRAWS_EVERY_STEP or any(r["elapsed_step"].min() == 0 for r in first), "no reset inside the window"
    state = h.pool.get_state()
    h.api.restore(blob)
    same_rows(h.run(acts), first, (tag, "host blob"))
    same_bits(h.pool.get_state(), state, (tag, "state, host blob"))
    ti.restore_device(h.pool, dblob)
    same_rows(h.run(acts), first, (tag, "device blob"))
    same_bits(h.pool.get_state(), state, (tag, "state, device blob"))
    # a copy of the device blob has lost the remembered header: restore_device reads it back from the device
    ti.restore_device(h.pool, dblob.clone())
    same_rows(h.run(acts[:2]), first[:2], (tag, "cloned device blob"))


@pytest.mark.parametrize("case", sorted(TASKS))
def test_whole_pool_continues_bit_for_bit(case):
    h = Handle(case, seed=7)
    continuation(h, case)
    h.close()


def into_another_pool(a, a_ids, b, twin, tag, device_blob=False):
    """Test 2's comparison: b.restore(a.snapshot(a_ids), IDS2); then b's rows IDS2 are a's rows a_ids in every key
    but the env ids, and b's other rows are those of its untouched twin.  `device_blob`: the blob stays on the device
    (snapshot_device / restore_device)."""
    rng = np.random.default_rng(5)
    if device_blob:
        from envpool_amd import torch_interop as ti

        dblob = ti.snapshot_device(a.pool, a_ids)
        assert dblob.numel() == a.pool.snapshot_bytes(len(a_ids))
        ti.restore_device(b.pool, dblob, IDS2 + b.pool.env_id_offset)
    else:
        blob = a.api.snapshot(a_ids)
        assert blob.nbytes == a.pool.snapshot_bytes(len(a_ids))
        b.api.restore(blob, IDS2 + b.pool.env_id_offset)
    others = np.setdiff1d(np.arange(b.n), IDS2)
    ra, rb, rt = [], [], []
    for _ in range(STEPS):
        act_a, act_b = a.actions(rng), b.actions(rng)
        ra.append(a.step(act_a))
        rt.append(twin.step(act_b))
        act_b = act_b.copy()
        act_b[IDS2] = act_a[a_ids - a.pool.env_id_offset]
        rb.append(b.step(act_b))
    same_rows(rb, ra, (tag, "restored rows"), IDS2, a_ids - a.pool.env_id_offset, skip=ID_KEYS)
    same_rows(rb, rt, (tag, "untouched rows"), others, others)
    for r in rb:
        same_bits(r["info:env_id"][:, 0], b.ids, (tag, "env ids stay the pool's own"))


@pytest.mark.parametrize("case", sorted(TASKS))
def test_subset_continues_in_another_pool(case):
    a, b, twin = Handle(case, seed=7), Handle(case, seed=1007), Handle(case, seed=1007)
    rng = np.random.default_rng(4)
    warm_up(a, rng)
    b.reset(), twin.reset()
    for _ in range(5):  # (B is elsewhere in its episodes, and in its generators' blocks)
        act = b.actions(rng)
        b.step(act), twin.step(act)
    into_another_pool(a, IDS, b, twin, case)
    for h in (a, b, twin):
        h.close()


# one id per way of drawing from the generator: CartPole NextWords bursts, Blackjack UniformInt, Pendulum UniformReal,
# HalfCheetah Normal, the Ant (its own kernel), Game2048 UniformInt + Canonical, Minesweeper a shuffle, the MiniGrid
# and PGX reset kernels
MIXED_LAYOUT_TASKS = ["CartPole-v1", "Blackjack-v1", "Pendulum-v1", "HalfCheetah-v4", "Ant-v4", "Game2048-v1",
                      "Minesweeper-v0", "MiniGrid-Dynamic-Obstacles-6x6-v0", "Othello-v1"]


def blob_generators(blob):
    """(generator layout, positions [k]) of a generator-carrying blob of a pool without a frame stack: the header
    fields and section offsets of envpool_amd/csrc/snapshot.hip.h (`struct Header`, `LayoutOf`)."""
    assert int(blob[:8].view("<u4")[1]) == 1, "snapshot.hip.h: kVersion has changed, and with it maybe the layout"
    dim, k, flags, shift, stack_s = (int(x) for x in blob[16:36].view("<i4"))
    assert flags & 1 and stack_s == 1
    off = (64 + 8 * k * dim + 63) // 64 * 64 + 4 * 624 * k
    return shift, blob[off:off + 4 * k].view("<i4").copy()


# CartPole draws 8 words per reset and no env falls within 6 steps: after warm_up's 12 steps every env has reset twice
# and stands at word 16, a tile start.  Three more steps bring the third reset (word 24).
MIXED_WARM_UP = {"CartPole-v1": STEPS + 3}


def mixed_layouts(task, tiles, device_blob):
    a = Handle(task, seed=7, engine_keys={"mt_tile": tiles[0]})
    b, twin = (Handle(task, seed=1007, engine_keys={"mt_tile": tiles[1]}) for _ in range(2))
    rng = np.random.default_rng(4)
    warm_up(a, rng, MIXED_WARM_UP.get(task, STEPS))
    b.reset(), twin.reset()
    for _ in range(5):
        act = b.actions(rng)
        b.step(act), twin.step(act)
    shift, mti = blob_generators(a.api.snapshot(IDS))
    assert shift == {1: 0, 16: 4}[tiles[0]]
    assert blob_generators(b.api.snapshot(IDS2))[0] == {1: 0, 16: 4}[tiles[1]]
    assert ((0 <= mti) & (mti < 624)).all()
    # inside a tile the two layouts hold different words: a blob whose positions all start a tile would restore
    # correctly as a verbatim copy, and the case would prove nothing
    assert (mti % 16 != 0).any(), mti
    into_another_pool(a, IDS, b, twin, (task, tiles), device_blob)
    for h in (a, b, twin):
        h.close()


@pytest.mark.parametrize("tiles", [(1, 16), (16, 1)])
@pytest.mark.parametrize("task", MIXED_LAYOUT_TASKS)
def test_subset_continues_in_a_pool_of_the_other_generator_layout(task, tiles):
    """A's generators are [624][N] and B's tiled, or the reverse ("mt_tile"): the restore converts the partly
    consumed tile of every env, so B's rows IDS2 continue as A's rows IDS do, resets and their draws included."""
    mixed_layouts(task, tiles, False)


@pytest.mark.parametrize("tiles", [(1, 16), (16, 1)])
def test_device_blob_moves_between_generator_layouts(tiles):
    mixed_layouts("Blackjack-v1", tiles, True)


@pytest.mark.parametrize("task", ["HalfCheetah-v4", "Ant-v4"])
def test_frame_stack_ring_is_part_of_the_snapshot(task):
    h = Handle(task, seed=7, frame_stack=3)
    plain = Handle(task, seed=7)
    assert h.pool.snapshot_bytes(N) > plain.pool.snapshot_bytes(N)
    continuation(h, (task, "frame_stack=3"))
    with pytest.raises(ValueError, match="frame_stack"):
        plain.api.restore(h.api.snapshot())
    with pytest.raises(ValueError, match="frame_stack"):
        h.api.restore(plain.api.snapshot())
    h.close(), plain.close()


@pytest.mark.parametrize("task", ["Game2048-v1", "HalfCheetah-v4"])
def test_without_the_generator_a_restore_is_set_state(task):
    h, twin = Handle(task, seed=7), Handle(task, seed=7)
    rng = np.random.default_rng(6)
    for x in (h, twin):
        warm_up(x, np.random.default_rng(6))
    rng = np.random.default_rng(8)
    blob = h.api.snapshot(rng=False)
    full = h.api.snapshot()
    # shorter by the generator section: 624 words and the position per env, rounded up to 64 bytes
    assert full.nbytes - blob.nbytes == (4 * 624 * N + 4 * N + 63) // 64 * 64
    assert blob.nbytes == h.pool.snapshot_bytes(N, rng=False)
    acts = [h.actions(rng) for _ in range(STEPS)]
    h.run(acts[:3])  # (the generators move on: the restore must not bring them back)
    twin.run(acts[:3])
    state = twin.pool.get_state()
    h.api.restore(h.api.snapshot(rng=False))
    twin.pool.set_state(state)
    same_rows(h.run(acts), twin.run(acts), (task, "rng=False"))
    # ... and a state from earlier with today's generators: set_state of that state
    h.api.restore(blob)
    twin.pool.set_state(np.frombuffer(blob, np.float64, N * h.pool.state_dim(), 64).reshape(N, -1))
    same_rows(h.run(acts), twin.run(acts), (task, "earlier state, rng=False"))
    h.close(), twin.close()


@pytest.mark.parametrize("task", ["Game2048-v1", "Othello-v1", "MiniGrid-Dynamic-Obstacles-6x6-v0"])
def test_fork(task):
    h, twin = Handle(task, seed=7), Handle(task, seed=7)
    for x in (h, twin):
        warm_up(x, np.random.default_rng(9))
    rng = np.random.default_rng(10)
    dst = np.arange(10, 20, dtype=np.int32)
    with pytest.raises(ValueError, match="twice"):
        h.api.fork([3, 4], [10, 10])
    with pytest.raises(ValueError):
        h.api.fork([3], [N])
    h.api.fork([3] * 10, dst)
    family = np.concatenate([[3], dst])
    others = np.setdiff1d(np.arange(N), dst)
    got, want = [], []
    for _ in range(STEPS):  # the same action in all eleven: one env eleven times, resets included
        act = h.actions(rng)
        want.append(twin.step(act))
        act = act.copy()
        act[dst] = act[3]
        got.append(h.step(act))
    assert task in DRAWS_EVERY_STEP or any(r["elapsed_step"][3, 0] == 0 for r in got), "no reset inside the window"
    for t, r in enumerate(got):
        for k, v in r.items():
            if k not in ID_KEYS:
                same_bits(v[family], np.repeat(v[3:4], len(family), axis=0), (task, t, k, "forked rows"))
    same_rows(got, want, (task, "untouched rows"), others, others)
    got, want = [], []
    for _ in range(6):  # different actions: the copies go their own ways, everybody else as in the twin
        act = h.actions(rng)
        want.append(twin.step(act))
        got.append(h.step(act))
    same_rows(got, want, (task, "untouched rows, own actions"), others, others)
    # swap two envs (targets overlap sources)
    h.api.fork([0, 1], [1, 0])
    got, want = [], []
    for _ in range(STEPS):
        act = h.actions(rng)
        want.append(twin.step(act))
        act = act.copy()
        act[[0, 1]] = act[[1, 0]]
        got.append(h.step(act))
    same_rows(got, want, (task, "swapped"), [0, 1], [1, 0], skip=ID_KEYS)
    h.close(), twin.close()


@pytest.mark.parametrize("task", ["CartPole-v1", "Game2048-v1"])
def test_snapshot_shows_sends_not_yet_received(task):
    """An async pool: the snapshot is taken between a send and its recv and shows the envs after that send."""
    a = Handle(task, seed=7, batch_size=N // 2)
    ref, sync = Handle(task, seed=7), Handle(task, seed=99)
    lo, hi = a.ids[:N // 2], a.ids[N // 2:]
    rng = np.random.default_rng(11)
    a.pool.reset(a.ids)
    a.rows(), a.rows()
    ref.reset(), sync.reset()
    for _ in range(STEPS):
        act = a.actions(rng)
        a.pool.send(lo, act[:N // 2])
        a.pool.send(hi, act[N // 2:])
        a.rows(), a.rows()
        ref.step(act)
    act = a.actions(rng)
    a.pool.send(lo, act[:N // 2])  # ... not received
    blob = a.api.snapshot()
    ref.step(act[:N // 2], lo)
    sync.api.restore(blob)
    acts = [a.actions(rng) for _ in range(STEPS)]
    same_rows(sync.run(acts), ref.run(acts), (task, "after the pending send"))
    pending = a.rows()
    assert np.array_equal(pending["info:env_id"][:, 0], lo)
    for h in (a, ref, sync):
        h.close()


@pytest.mark.parametrize("task", ["CartPole-v1", "Othello-v1"])
def test_last_rows_of_a_big_pool(task):
    big_n = 65536
    a = Handle(task, seed=7, n=big_n)
    b, twin = Handle(task, seed=1007), Handle(task, seed=1007)
    warm_up(a, np.random.default_rng(12))
    for x in (b, twin):
        warm_up(x, np.random.default_rng(13), steps=5)
    into_another_pool(a, np.arange(big_n - 6, big_n, dtype=np.int32), b, twin, task)
    for h in (a, b, twin):
        h.close()


def test_refusals():
    cart, pend = Handle("CartPole-v1", seed=7), Handle("Pendulum-v1", seed=7)
    shard = Handle("CartPole-v1", seed=7, env_id_offset=100)
    for h in (cart, pend, shard):
        warm_up(h, np.random.default_rng(14), steps=3)
    blob = cart.api.snapshot(IDS)
    with pytest.raises(ValueError, match="another env family"):
        pend.api.restore(blob, IDS2)
    with pytest.raises(ValueError, match="shorter than its header"):
        cart.api.restore(blob[:-64], IDS2)
    with pytest.raises(ValueError, match="shorter than a header"):
        cart.api.restore(blob[:40], IDS2)
    with pytest.raises(ValueError, match="another number of envs"):
        cart.api.restore(blob, IDS2[:5])
    with pytest.raises(ValueError, match="twice"):
        cart.api.restore(blob, [1, 2, 3, 4, 5, 1])
    with pytest.raises(ValueError, match="out of range"):
        cart.api.snapshot([N])
    # ids are global: a pool that is a shard of a bigger one knows its envs as 100 .. 139
    with pytest.raises(ValueError, match="out of range"):
        shard.api.restore(blob, IDS2)
    shard.api.restore(blob, IDS2 + 100)
    same_bits(shard.pool.get_state(IDS2 + 100), cart.pool.get_state(IDS), "restored into a shard")
    # env_ids=None: envs 0 .. k-1 of the target, k from the blob
    pend_state, want = pend.pool.get_state(), cart.pool.get_state(IDS)
    cart.api.restore(blob)
    same_bits(cart.pool.get_state(np.arange(6)), want, "restore without ids")
    same_bits(pend.pool.get_state(), pend_state, "a refused blob changes nothing")
    for h in (cart, pend, shard):
        h.close()


def test_atari_refuses_snapshots():
    import ctypes

    from atari_util import plugin_path, register_synthetic_ids

    register_synthetic_ids()
    env = envpool.make("SynthFire-v5", env_type="gymnasium", num_envs=4, seed=1, emulator_lib=plugin_path(),
                       base_path="/synthetic")
    env.reset()
    pool = env.device_pool
    header = np.zeros(64, np.uint8)
    header[20:24].view("<i4")[0] = 1
    header[48:56].view("<u8")[0] = 64
    spare = ctypes.create_string_buffer(256)
    addr = (ctypes.addressof(spare) + 15) // 16 * 16  # (never dereferenced: the pool refuses first)
    msg = "snapshot not implemented for this environment"
    for call in (lambda: pool.snapshot_bytes(1), lambda: env.snapshot(), lambda: env.snapshot([0], rng=False),
                 lambda: env.restore(header, [0]), lambda: env.fork([0], [1]),
                 lambda: pool.snapshot_device(addr, [0]), lambda: pool.restore_device(addr, header.tobytes(), [0])):
        with pytest.raises(RuntimeError, match=msg):
            call()
    env.close()


def test_sharded_pool_restores_shard_by_shard():
    env = envpool.make_gym("HalfCheetah-v4", num_envs=N, seed=7, max_episode_steps=6, device=[0, 0])
    rng = np.random.default_rng(15)
    env.reset()
    for _ in range(STEPS):
        env.step(rng.uniform(-1, 1, (N, 6)))
    blobs = env.snapshot()
    assert isinstance(blobs, list) and len(blobs) == 2
    acts = [rng.uniform(-1, 1, (N, 6)) for _ in range(STEPS)]

    def flat(d, prefix):
        out = {}
        for k, v in d.items():
            out.update(flat(v, prefix + k + ".") if isinstance(v, dict) else {prefix + k: v})
        return out

    def run():
        out = []
        for a in acts:
            obs, rew, term, trunc, info = env.step(a)
            out.append({"obs": obs, "rew": rew, "term": term, "trunc": trunc, **flat(info, "info:")})
        return [{k: np.array(v).reshape(N, -1) for k, v in r.items()} for r in out]

    first = run()
    assert any(r["info:elapsed_step"].min() == 0 for r in first)
    env.restore(blobs)
    same_rows(run(), first, "sharded")
    with pytest.raises(ValueError, match="env_ids"):
        env.snapshot(np.arange(4))
    with pytest.raises(ValueError, match="env_ids"):
        env.restore(blobs, np.arange(N))
    with pytest.raises(ValueError, match="across shards"):
        env.fork([0], [N - 1])
    env.fork([0], [1])
    env.close()
