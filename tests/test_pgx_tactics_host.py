"""PGX guided search, exact leaf status, CPU side: the new pieces of envpool_amd/csrc/pgx_guided.hip.h built for the
host by g++ (tests/cpu_harness/pgx_tactics_host.cpp: the wide harness's session plus the solver stage, a wave's lanes as
loops) against the numpy restatements driven through subclasses that decide every new status-0 leaf with the
brute-force minimax (pgx_tactics_util.py) -- call for call in status, obs, mask, the result and `decided`, under the
stand-in and the constant evaluator, with the coverage conditions asserted per game; tactics = 0 against the existing
harnesses; reroot onto a decided child, onto a subtree that holds one, onto an untried move; a tight node budget; the
stand-alone program under the host sanitizers; and the argument checks of the Python layers, which come before any
native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_tactics_util as U
import test_pgx_guided_host as plain

F = np.float32


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_tactics")
    out = U.build_libs(tmp)
    out["guided"] = ctypes.CDLL(U.compile_harness(tmp, "pgx_guided_host.cpp"))
    out["guided"].pgx_guided_begin.restype = ctypes.c_void_p
    out["guided"].pgx_guided_result.restype = None
    out["guided"].pgx_guided_end.restype = None
    out["tmp"] = tmp
    return out


_roots = {}


def roots_of(libs, fam):
    if fam not in _roots:
        game = U.Game(libs, fam)
        _roots[fam] = (game, U.root_set(libs, game))
    return _roots[fam]


# ---- harness == restatement, with the coverage ----------------------------------------------------------------------
@pytest.mark.parametrize("evaluator", ["stand_in", "constant"])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fam", U.GAMES)
def test_harness_equals_the_restatement_with_brute_force_decisions(libs, fam, wide, evaluator):
    game, roots = roots_of(libs, fam)
    W = U.WIDTH[fam] if wide else 1
    assert roots[-2].done and roots[-1].mask.sum() == 1 and not roots[-1].done
    total = {"+1": 0, "-1": 0, "eval": 0, "native": 0}
    for depth in U.DEPTHS[fam]:
        pair = U.Pair(libs, game, roots, U.SIMS[fam], W, depth, evaluator)
        visits, _, action, _, done = pair.round()
        for k, v in pair.events().items():
            total[k] += v
        decided, nodes, _ = pair.host.decided()
        running = np.array([not r.done for r in roots])
        assert (visits[running].sum(1) == U.SIMS[fam]).all() and not visits[~running].any()
        assert (action[~running] == -1).all() and (decided[~running] == 0).all()
        assert (nodes >= decided).all() and nodes[running].sum() > 0  # the solver ran, on running roots only
        assert (nodes[~running] == 0).all()
        if wide:
            assert pair.calls < U.SIMS[fam] + 1
        only = int(np.flatnonzero(roots[-1].mask)[0])  # the single-move root: collisions, or slots on one finished game
        assert visits[-1][only] == U.SIMS[fam] and action[-1] == only
        pair.close()
    # the coverage is a condition: a leaf decided +1, one decided -1, an evaluated leaf, a native finished-game leaf
    assert min(total.values()) >= 1, (fam, W, evaluator, total)


# ---- tactics = 0 is today's session ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", U.GAMES)
def test_tactics_0_equals_the_plain_and_the_wide_harness_byte_for_byte(libs, fam):
    game, roots = roots_of(libs, fam)
    S = U.SIMS[fam]
    for W in (1, U.WIDTH[fam]):
        off = U.TacticsHost(libs, fam, roots, S, W, 0)
        old = U.TacticsHost(libs, fam, roots, S, W, 0, plain=True)
        guided = plain.HostSession((None, libs["guided"]), f"{fam}-v1", roots, S, U.C_PUCT) if W == 1 else None
        for t in range(S + 1):
            got, ref = off.leaves(), old.leaves()
            for x, y in zip(got, ref):
                assert np.array_equal(x, y), (fam, W, t)
            priors, values = U.stand_in_rows(got[0], got[1])
            assert off.advance(priors, values) == 0 and old.advance(priors, values) == 0
            for x, y in zip(off.result(), old.result()):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (fam, W, t)
            if guided is not None:
                for x, y in zip(got, guided.leaves()):
                    assert np.array_equal(x[:, 0], y), (fam, t)
                assert guided.advance(priors[:, 0], values[:, 0]) == 0
                for x, y in zip(off.result()[:4], guided.result()):
                    assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (fam, t)
        decided, nodes, _ = off.decided()
        assert not decided.any() and not nodes.any()
        off.close()
        old.close()
        if guided is not None:
            guided.close()


# ---- reroot ---------------------------------------------------------------------------------------------------------
def _subtree_has_decided(tree, c):
    stack = [ch for ch in tree.nodes[c]["child"] if ch >= 0]
    while stack:
        k = stack.pop()
        if tree.nodes[k].get("decided"):
            return True
        stack.extend(ch for ch in tree.nodes[k]["child"] if ch >= 0)
    return False


def _choose(pair, order):
    """Per root a move to play, by the first kind of `order` the root offers: onto a decided child, onto an undecided
    child whose kept subtree holds a decided node, onto an untried move.  Returns (actions, the kind per root)."""
    actions, kinds = [], []
    for i, tree in enumerate(pair.trees):
        n0, found = tree.nodes[0], {}
        for a in ([] if tree.over else [int(a) for a in np.flatnonzero(n0["pos"].mask)]):
            c = n0["child"][a]
            kind = ("untried" if c < 0 else "decided" if tree.nodes[c].get("decided")
                    else "kept" if _subtree_has_decided(tree, c) else "other")
            found.setdefault(kind, a)
        want = order[i % len(order):] + order[:i % len(order)] + ["other", "decided", "kept", "untried"]
        kind = next((k for k in want if k in found), None)
        actions.append(found[kind] if kind else 0)
        kinds.append(kind)
    return actions, kinds


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fam", ["TicTacToe", "ConnectFour"])
def test_reroot_onto_a_decided_child_a_kept_decided_node_and_an_untried_move(libs, fam, wide):
    """Three rounds with two reroots: the first onto decided children and onto subtrees that hold a decided node, the
    second -- after a short round, which leaves root moves untried -- onto untried moves.  Harness and restatement are
    compared after every call, the reroots included."""
    game, roots = roots_of(libs, fam)
    S, W, D = U.SIMS[fam], (U.WIDTH[fam] if wide else 1), 2
    pair = U.Pair(libs, game, roots, S, W, D, "stand_in", nodes=3 * S + 1)
    pair.round()
    before = pair.host.decided()[0].copy()
    actions, kinds = _choose(pair, ["decided", "kept"])
    assert kinds.count("decided") >= 1 and kinds.count("kept") >= 1, kinds
    pair.reroot(actions, 3)
    status, res = pair.host.status, pair.host.result()
    for i, kind in enumerate(kinds):
        if kind == "decided":  # a decided node that becomes the root runs on: status 0, counted in result
            assert status[i, 0] == 0 and res[2][i] != -1 and not pair.trees[i].over
            assert not pair.trees[i].nodes[0].get("decided")
        if kind == "kept":  # the decided node deeper in the kept subtree stays decided
            assert status[i, 0] == 0 and any(nd.get("decided") for nd in pair.trees[i].nodes[1:])
    assert np.array_equal(pair.host.decided()[0], before)  # reroot does not reduce the counters
    pair.round()
    middle = pair.host.decided()[0].copy()
    assert (middle >= before).all()
    actions, kinds = _choose(pair, ["untried"])
    assert kinds.count("untried") >= 1, kinds
    pair.reroot(actions, 6)
    for i, kind in enumerate(kinds):
        if kind == "untried":  # a fresh, undecided root
            assert len(pair.trees[i].nodes) == 1 and not pair.trees[i].nodes[0].get("decided")
    pair.round()
    assert (pair.host.decided()[0] >= middle).all()
    pair.close()


# ---- a tight budget -------------------------------------------------------------------------------------------------
def _tight_run(libs, fam, roots, S, W, D, M):
    host = U.TacticsHost(libs, fam, roots, S, W, D, M)
    rec, given, marked_given = [], 0, 0
    for t in range(S + 1):
        leaves = host.leaves()
        if (leaves[2] == 2).all():
            break
        priors, values = U.stand_in_rows(leaves[0], leaves[1])
        assert host.advance(priors, values) == 0
        decided, nodes, gave_up = host.decided()
        given += int(gave_up.sum())
        marked_given += int((host.status[gave_up != 0] != 0).sum())  # a given-up leaf stays a status-0 leaf
        rec.append([x.copy() for x in host.leaves()] + list(host.result()) + [decided, nodes])
    host.close()
    return rec, given, marked_given


def test_a_tight_budget_gives_leaves_up_deterministically_and_marks_none_of_them(libs):
    fam, D, M = "ConnectFour", 4, 64
    game, roots = roots_of(libs, fam)
    S, W = U.SIMS[fam], U.WIDTH[fam]
    first, given, marked = _tight_run(libs, fam, roots, S, W, D, M)
    assert given > 0 and marked == 0
    again, _, _ = _tight_run(libs, fam, roots, S, W, D, M)
    perm = np.random.default_rng(3).permutation(len(roots))
    permuted, _, _ = _tight_run(libs, fam, [roots[i] for i in perm], S, W, D, M)
    assert len(first) == len(again) == len(permuted)
    for a, b, c in zip(first, again, permuted):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
            assert np.array_equal(x[perm].view(np.uint8), z.view(np.uint8))
    roomy, given_roomy, _ = _tight_run(libs, fam, roots, S, W, D, U.BIG)
    assert given_roomy == 0 and roomy[-1][-2].sum() > first[-1][-2].sum()  # M = 2^20 gives nothing up and decides more


# ---- the stand-alone program under the host sanitizers --------------------------------------------------------------
def test_the_stand_alone_program_runs_clean_under_the_host_sanitizers(libs):
    exe = U.compile_harness(libs["tmp"], "pgx_tactics_host.cpp", shared=False,
                            flags=("-DPGX_TACTICS_MAIN", "-g", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=undefined"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 12 and "ERROR" not in out.stderr and "runtime error" not in out.stderr
    assert any(" 0 decided" not in ln for ln in lines)  # the rounds decided something


# ---- the header's limits, the C ABI, the Python layers --------------------------------------------------------------
def test_limits_and_symbols(libs):
    from envpool_amd.core import native

    lim = libs["tactics"].pgx_tactics_limits
    assert (lim(0), lim(1), lim(2)) == (native.GUIDED_MAX_TACTICS, native.GUIDED_MAX_TACTICS_NODES, 2)
    header = open(os.path.join(U.ROOT, "include", "envpool_amd.h")).read()
    for name in ("epa_guided_begin_tactics", "epa_guided_begin_tactics_device", "epa_guided_decided",
                 "epa_guided_decided_device"):
        assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header
    assert "#define EPA_GUIDED_MAX_TACTICS 16" in header and "#define EPA_GUIDED_TACTICS_NODES 4096" in header
    game, roots = roots_of(libs, "TicTacToe")
    for tactics, m in ((17, 64), (-1, 64), (2, 0), (2, (1 << 20) + 1)):
        U.TacticsHost(libs, "TicTacToe", roots[:1], 4, 1, tactics, m, want_rc=-6)


def test_check_guided_tactics():
    from envpool_amd.core import native

    assert native.check_guided_tactics(0, 4096) == (0, 4096) and native.check_guided_tactics(None, 1) == (0, 1)
    assert native.check_guided_tactics(16, 1 << 20) == (16, 1 << 20)
    assert native.check_guided_tactics(np.int64(3), np.int32(64)) == (3, 64)
    for bad in (17, -1, 2.5, True):
        with pytest.raises(ValueError, match="guided_begin: tactics = "):
            native.check_guided_tactics(bad, 4096)
    for bad in (0, (1 << 20) + 1, -5, 1.5, True):
        with pytest.raises(ValueError, match="guided_begin: tactics_nodes"):
            native.check_guided_tactics(2, bad)


class _Recorder(plain._Recorder):
    def guided_begin(self, env_ids, simulations, c_puct, *more):
        out = super().guided_begin(env_ids, simulations, c_puct)
        if more:
            self.calls[-1] += more
        return out

    def guided_decided(self):
        self.calls.append(("decided",))
        return np.zeros(self.k, np.int32)


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    for kw in (dict(tactics=17), dict(tactics=-1), dict(tactics=1.5), dict(tactics=2, tactics_nodes=0),
               dict(tactics=2, tactics_nodes=(1 << 20) + 1)):
        with pytest.raises(ValueError, match="guided_begin: tactics"):
            env.guided_search(ids, simulations=8, **kw)
    with pytest.raises(ValueError, match="tactics is an argument of policy='puct'"):
        env.guided_search(ids, simulations=8, policy="gumbel", tactics=2)
    with pytest.raises(ValueError, match="gumbel_search: tactics"):
        env.gumbel_search(ids, simulations=8, tactics=2)
    assert env._pool.calls == []
    # the default is today's calls
    gs = env.guided_search(ids, simulations=3, c_puct=0.5, tactics=0)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5)] and gs.tactics == 0
    gs.close()
    env._pool.calls.clear()
    gs = env.guided_search(ids, simulations=3, c_puct=0.5, tactics=2)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5, 0, None, 2, 4096)] and gs.tactics == 2
    assert gs.decided.tolist() == [0, 0, 0] and env._pool.calls[-1] == ("decided",)
    gs.close()
    with pytest.raises(ValueError, match="closed"):
        gs.decided
    env._pool.calls.clear()
    gs = env.guided_search(ids, simulations=3, c_puct=0.5, nodes=9, width=4, tactics=16, tactics_nodes=64)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5, 9, 4, 16, 64)] and gs.width == 4
    gs.close()
