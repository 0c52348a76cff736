"""The PGX rules at crafted positions on the MI355X: the gfx950 step kernel against the scalar restatement of the
rules (pgx_rules_ref.py, pinned to the reference by the fixtures in test_pgx_rules_host.py) at the position families
of pgx_rules_families.py.  A family's rows go into a pool of at most 8192 envs in batches through set_state as
[elapsed, done, hidden words], then one send / recv_dict / get_state; every key and the hidden words must be equal."""
import numpy as np
import pytest

import pgx_rules_families as F
import pgx_rules_ref as R
from envpool_amd.core.device_pool import DevicePool
from pgx_util import KEYS, PER_PLAYER

pytestmark = pytest.mark.gpu

POOL = 8192


def device_step(name):
    fam, want, _ = F.family(name)
    n = len(fam["actions"])
    size = min(POOL, n)
    pool = DevicePool(fam["game"], size, seed=1, max_episode_steps=int(fam["limit"]))
    ids = np.arange(size, dtype=np.int32)
    pool.reset(ids)
    pool.recv_dict()
    outs = {k: np.zeros_like(want[k]) for k in KEYS}
    hid = np.zeros((n, R.hidden_words(fam["game"])), np.int64)
    for start in range(0, n, size):
        rows = (start + np.arange(size)) % n  # the last batch is filled up from the family's first rows
        k = min(size, n - start)
        state = np.zeros((size, 2 + fam["hidden"].shape[1]))
        state[:, 0] = fam["elapsed"][rows]
        state[:, 2:] = fam["hidden"][rows]
        pool.set_state(state)
        pool.send(ids, fam["actions"][rows])
        out = pool.recv_dict()
        after = pool.get_state()
        for key in KEYS:
            got = np.asarray(out[key])
            assert got.shape[0] == (2 * size if key in PER_PLAYER else size), (name, key, got.shape)
            if key in ("info:env_id", "info:players.env_id"):
                got = got + start
            outs[key][start:start + k] = got.reshape(size, -1)[:k].reshape(outs[key][start:start + k].shape)
        assert np.array_equal(after[:k, 0], fam["elapsed"][rows[:k]] + 1), name
        assert np.array_equal(after[:k, 1] != 0, outs["done"][start:start + k]), name
        hid[start:start + k] = after[:k, 2:]
    pool.close()
    return outs, hid


@pytest.mark.parametrize("name", sorted(F.FAMILIES))
def test_kernel_agrees_with_restatement(name):
    outs, hid = device_step(name)
    assert F.differences(name, outs, hid) == [], name
