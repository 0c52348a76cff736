"""Every entry point that opens a guided-search session opens the SAME session: epa_guided_begin and its _nodes, _wide,
_tactics and _prove forms with the later options at their defaults, host form and _device twin, compared with each other
bit for bit -- the leaves of every advance and the final result arrays; the wide forms among themselves at width 2; and
epa_gumbel_begin (a plain session) and epa_gumbel_begin_batch (batch 2), which have no default in common, each with its
_device twin.  No reference: the oracle tests of the single forms pin the values, this file pins that the forms agree.
Every session is a handful of launches on 3 roots."""
import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native

pytestmark = pytest.mark.gpu

F = np.float32
K, S, C_PUCT = 3, 4, 1.25
CONSIDERED, C_VISIT, C_SCALE = 4, 50.0, 0.1
GAMES = ("TicTacToe", "ConnectFour")
PLIES = 3


@pytest.fixture(scope="module", params=GAMES)
def pool(request):
    """3 envs, stepped 3 fixed plies: env i plays its (i + ply)-th legal action, so the rows differ."""
    env = envpool.make(f"{request.param}-v1", "gymnasium", num_envs=K, seed=11)
    _, info = env.reset()
    for ply in range(PLIES):
        mask = np.asarray(info["legal_action_mask"], bool)
        act = [np.flatnonzero(m)[(i + ply) % m.sum()] for i, m in enumerate(mask)]
        _, _, _, _, info = env.step(np.asarray(act, np.int32))
    yield env.device_pool
    env.close()


class Host:
    """The arrays of a host form: numpy."""

    def __init__(self, pool):
        pass

    def empty(self, shape, dtype):
        return np.zeros(shape, dtype)

    def put(self, x):
        return np.ascontiguousarray(x)

    def ptr(self, x):
        return x.ctypes.data

    def get(self, x):
        return x.copy()


class Device:
    """The arrays of a _device twin: torch tensors on the pool's device.  The calls only enqueue on the pool's stream,
    so the whole device is synchronised before the host reads or rewrites what a call uses."""

    def __init__(self, pool):
        import torch

        self.torch, self.dev = torch, torch.device("cuda", pool.device)

    def empty(self, shape, dtype):
        t = self.torch.zeros(shape, dtype=getattr(self.torch, np.dtype(dtype).name), device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        return t

    def put(self, x):
        t = self.torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        self.torch.cuda.synchronize(self.dev)
        return t

    def ptr(self, x):
        return x.data_ptr()

    def get(self, x):
        self.torch.cuda.synchronize(self.dev)
        return x.cpu().numpy()


def _round(pool, mem, rows, begin, policy, extra_result):
    """One round to its end: `begin(obs, mask, status)` opens the session, then up to S + 1 advances answered by the
    fixed evaluator (uniform priors over the mask -- for the Gumbel policy uniform logits --, value 0), a plain session
    all of them, a session with slots until no slot is pending; then the result.  Returns every array on the way."""
    lib, h = pool._lib, pool._h
    hh, ww, cc, a = pool.guided_shape()
    suffix = "_device" if isinstance(mem, Device) else ""
    obs, mask = mem.empty((rows, hh, ww, cc), np.uint8), mem.empty((rows, a), np.uint8)
    status = mem.empty(rows, np.uint8)
    out = []
    begin(suffix, mem, mem.ptr(obs), mem.ptr(mask), mem.ptr(status))
    out += [mem.get(obs), mem.get(mask), mem.get(status)]
    advance = getattr(lib, f"epa_{policy}_advance{suffix}")
    for _ in range(S + 1):
        if rows != K and (out[-1] == 2).all():
            break
        legal = out[-2].astype(F)
        if policy == "guided":
            answer = legal / np.maximum(legal.sum(1, keepdims=True), 1)
        else:
            answer = np.zeros_like(legal)
        d_answer, d_values = mem.put(answer.astype(F)), mem.put(np.zeros(rows, F))
        native.check(advance(h, mem.ptr(d_answer), mem.ptr(d_values), rows, mem.ptr(obs), mem.ptr(mask),
                             mem.ptr(status)))
        out += [mem.get(obs), mem.get(mask), mem.get(status)]
    assert rows == K or (out[-1] == 2).all()
    res = [mem.empty((K, a), np.int32), mem.empty((K, a), F), mem.empty(K, np.int32)]
    res += [mem.empty((K, a), F)] * extra_result
    native.check(getattr(lib, f"epa_{policy}_result{suffix}")(h, *[mem.ptr(x) for x in res]))
    out += [mem.get(x) for x in res]
    native.check(lib.epa_guided_end(h))
    return out


def _same(sessions):
    name0, first = sessions[0]
    assert any(x.any() for x in first[-3:]), "the searches found nothing"
    for name, other in sessions[1:]:
        assert len(other) == len(first), (name0, name)
        for i, (x, y) in enumerate(zip(first, other)):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name0, name, i)


def _puct_forms(pool, width):
    """(name, begin(suffix, mem, obs, mask, status)) for every entry point that can open a session of this width, every
    later option at its default.  epa_guided_begin_wide takes a width of 1 .. 32, never 0: its plain session is
    width 1, which is the plain session call for call (pgx_guided.hip.h), with one row per root."""
    ids = np.arange(K, dtype=np.int32)
    lib, h, m = pool._lib, pool._h, native.GUIDED_TACTICS_NODES

    def form(name, *options):
        def begin(suffix, mem, *leaves):
            native.check(getattr(lib, name + suffix)(h, ids.ctypes.data, K, S, *options, *leaves))
        return name, begin

    forms = [form("epa_guided_begin_wide", 0, width or 1, C_PUCT),
             form("epa_guided_begin_tactics", 0, width, C_PUCT, 0, m),
             form("epa_guided_begin_prove", 0, width, C_PUCT, 0, m, 0)]
    if width == 0:  # (a wide session cannot be opened through these two)
        forms = [form("epa_guided_begin", C_PUCT), form("epa_guided_begin_nodes", S + 1, C_PUCT)] + forms
    return forms


def test_puct_forms_open_the_same_plain_session(pool):
    """epa_guided_begin, _nodes (nodes = simulations + 1), _wide (nodes = 0), _tactics (tactics = 0) and _prove
    (flags = 0), each in its host form and its _device twin."""
    sessions = [(name + type(mem).__name__, _round(pool, mem, K, begin, "guided", 0))
                for name, begin in _puct_forms(pool, 0) for mem in (Host(pool), Device(pool))]
    assert len(sessions) == 10
    _same(sessions)


def test_puct_forms_open_the_same_wide_session(pool):
    """_wide, _tactics and _prove at width 2, each in its host form and its _device twin."""
    sessions = [(name + type(mem).__name__, _round(pool, mem, K * 2, begin, "guided", 0))
                for name, begin in _puct_forms(pool, 2) for mem in (Host(pool), Device(pool))]
    assert len(sessions) == 6
    _same(sessions)


@pytest.mark.parametrize("batch", [0, 2])
def test_gumbel_forms_agree_with_their_device_twins(pool, batch):
    """epa_gumbel_begin (a plain session) and epa_gumbel_begin_batch (batch 2: it takes 1 .. 32, and a batch session
    is not a plain one) against their _device twins; fixed non-zero noise."""
    ids = np.arange(K, dtype=np.int32)
    lib, h, a = pool._lib, pool._h, pool.guided_shape()[3]
    noise = np.random.default_rng(5).gumbel(size=(K, a)).astype(F)
    name = "epa_gumbel_begin_batch" if batch else "epa_gumbel_begin"
    options = (CONSIDERED, batch) if batch else (CONSIDERED,)

    def begin(suffix, mem, *leaves):
        d_noise = mem.put(noise)
        native.check(getattr(lib, name + suffix)(h, ids.ctypes.data, K, S, *options, C_VISIT, C_SCALE,
                                                 mem.ptr(d_noise), *leaves))
        mem.get(d_noise)  # (the noise stays alive until the launch that reads it is over)

    _same([(name + type(mem).__name__, _round(pool, mem, K * max(batch, 1), begin, "gumbel", 1))
           for mem in (Host(pool), Device(pool))])
