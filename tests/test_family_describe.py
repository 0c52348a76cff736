"""The C ABI's family list and key descriptions, pinned to tests/golden/family_describe.json
(tests/golden/make_family_describe.py): family order and names, player counts, and per family and per registered
task id the state keys, their player counts and the action keys.  An unknown family name fails the same way in every
entry point that takes one.  On the GPU: a created pool reports the keys the family describes."""
import ctypes
import json
import os
import sys

import pytest

from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_family_describe  # noqa: E402

with open(os.path.join(HERE, "golden", "family_describe.json")) as _f:
    GOLDEN = json.load(_f)


def test_family_table_matches_fixture():
    got = make_family_describe.collect()
    assert [f["name"] for f in got["families"]] == [f["name"] for f in GOLDEN["families"]]
    for g, want in zip(got["families"], GOLDEN["families"]):
        assert g == want, want["name"]
    assert native.lib().epa_family_name(len(GOLDEN["families"])) is None
    assert native.lib().epa_family_name(-1) is None


def test_task_descriptions_match_fixture():
    got = make_family_describe.collect()["tasks"]
    assert sorted(got) == sorted(GOLDEN["tasks"])
    for task_id, want in GOLDEN["tasks"].items():
        assert got[task_id] == want, task_id


def test_unknown_family_fails_everywhere():
    L = native.lib()
    name = b"NoSuchFamily"
    msg = "unknown env family: NoSuchFamily"
    cfg, keep = native.make_config(1)
    keys = (native.EpaKeyInfo * 32)()
    players = (ctypes.c_int32 * 32)()
    n = ctypes.c_int32(0)
    p = ctypes.c_int32(0)
    pool = ctypes.c_void_p()
    calls = {
        "epa_describe_state": lambda: L.epa_describe_state(name, ctypes.byref(cfg), keys, 32, ctypes.byref(n)),
        "epa_describe_action": lambda: L.epa_describe_action(name, ctypes.byref(cfg), keys, 32, ctypes.byref(n)),
        "epa_describe_state_players": lambda: L.epa_describe_state_players(name, ctypes.byref(cfg), players, 32,
                                                                           ctypes.byref(n)),
        "epa_family_players": lambda: L.epa_family_players(name, ctypes.byref(p)),
        "epa_create": lambda: L.epa_create(name, ctypes.byref(cfg), ctypes.byref(pool)),
    }
    for what, call in calls.items():
        code = call()
        assert code == native.EPA_ERR_INVALID, what
        assert L.epa_last_error().decode() == msg, what
        with pytest.raises(ValueError, match=f"^{msg}$"):
            native.check(code)
    assert not pool.value
    del keep


@pytest.mark.gpu
def test_pool_keys_match_description():
    """For every family of the table: a pool of 4 envs with the params of the family's first registered id (MiniGrid
    refuses an empty config) reports the state and action keys that epa_describe_* give for the same params."""
    params = {}
    for t in GOLDEN["tasks"].values():
        params.setdefault(t["family"], t["params"])
    for i in range(native.lib().epa_num_families()):
        family = native.lib().epa_family_name(i).decode()
        pool = DevicePool(family, 4, seed=0, params=params[family])
        try:
            for which in ("state", "action"):
                assert native.pool_keys(pool._h, which) == native.describe(family, params[family], which), \
                    (family, which)
        finally:
            pool.close()
