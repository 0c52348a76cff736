"""PGX guided search, proven values, CPU side: the new pieces of envpool_amd/csrc/pgx_guided.hip.h built for the host by
g++ (tests/cpu_harness/pgx_prove_host.cpp: the tactics harness's session with the climb, the closed picks, the proven
root and the proof read-out, a wave's lanes as loops) against the numpy restatements of rules 1 .. 9
(pgx_prove_util.py) -- call for call in status, obs, mask, the result, `proof` and `decided`, under the stand-in and the
constant evaluator, plain and W = 4, D = 0 and D = 2, with reroots; every proof against the brute force's full solve of
the root; the coverage conditions asserted on the restatement alone; a session without the flag against the existing
harnesses; the stand-alone program under the host sanitizers; and the argument checks of the Python layers, which come
before any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_prove_util as U
import pgx_tactics_util as T
import test_pgx_guided_host as plain

F = np.float32
WIDE = 4
DEPTHS = (0, 2)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_prove")
    out = U.build_libs(tmp)
    out["guided"] = ctypes.CDLL(U.compile_harness(tmp, "pgx_guided_host.cpp"))
    out["guided"].pgx_guided_begin.restype = ctypes.c_void_p
    out["guided"].pgx_guided_result.restype = None
    out["guided"].pgx_guided_end.restype = None
    out["tmp"] = tmp
    return out


_roots = {}
_seen = {}


def roots_of(libs, fam):
    if fam not in _roots:
        game = U.Game(libs, fam)
        roots = U.root_set(libs, game)
        _roots[fam] = (game, roots, U.truth(libs, game, roots))
    return _roots[fam]


def check_truth(pair, truth, what):
    """Every proof of the session against the brute force's full solve of the root."""
    value, q = pair.host.proof()
    proven = 0
    for i, t in enumerate(truth):
        if t is None or pair.trees[i].over:
            assert value[i] == U.UNPROVEN and (q[i] == U.UNPROVEN).all()
            continue
        if value[i] != U.UNPROVEN:
            proven += 1
            assert value[i] == t[0], (what, i, value[i], t[0])
        known = q[i] != U.UNPROVEN
        assert np.array_equal(q[i][known], t[1][known]), (what, i, q[i], t[1])
    return proven


# ---- harness == restatement == the truth, with the coverage ---------------------------------------------------------
@pytest.mark.parametrize("evaluator", ["stand_in", "constant"])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fam", U.GAMES)
def test_harness_equals_the_restatement_and_every_proof_is_true(libs, fam, wide, evaluator):
    game, roots, truth = roots_of(libs, fam)
    W, S = (WIDE if wide else 1), U.SIMS[fam]
    running = np.array([not r.done for r in roots])
    seen = _seen.setdefault(fam, dict.fromkeys(U.EVENTS, 0))
    for depth in DEPTHS:
        pair = U.ProvePair(libs, game, roots, S, W, depth, evaluator)
        visits, _, action, _, done = pair.round()
        proven = check_truth(pair, truth, (fam, W, depth))
        value, q = pair.host.proof()
        for i in np.flatnonzero(running):
            assert visits[i].sum() == done[i] <= S
            if value[i] == U.UNPROVEN:  # an unproven root ran its whole round
                assert done[i] == S
            else:  # the move played keeps the proven value
                assert q[i][action[i]] == value[i], (fam, i)
            if (q[i][roots[i].mask] != -1).any():  # never a move proven to lose while another is not
                assert q[i][action[i]] != -1
            seen["early"] += bool(value[i] != U.UNPROVEN and visits[i].sum() < S)
        assert not visits[~running].any() and (action[~running] == -1).all()
        assert proven >= 1
        for k, v in pair.seen().items():
            if k != "early":
                seen[k] += v
        pair.close()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fam", U.GAMES)
def test_reroot_onto_marked_nodes_keeps_marks_and_proves_the_new_root_at_once(libs, fam, wide):
    """Three rounds with two reroots, by turns onto marked children and onto subtrees that hold marked nodes deeper
    down, where a root offers one.  Harness and restatement are compared after every call, the reroots included, and
    the proofs of the first round against the truth."""
    game, roots, truth = roots_of(libs, fam)
    W, S = (WIDE if wide else 1), U.SIMS[fam]
    seen = _seen.setdefault(fam, dict.fromkeys(U.EVENTS, 0))
    for depth in DEPTHS:
        pair = U.ProvePair(libs, game, roots, S, W, depth, "stand_in", nodes=3 * S + 1)
        res = pair.round()
        check_truth(pair, truth, (fam, W, depth))
        for r, s2 in enumerate((S // 2, S)):
            actions = [t.reroot_choice(("deeper", "onto")[(i + r) % 2], int(res[2][i]))
                       for i, t in enumerate(pair.trees)]
            onto = [not t.over and t.nodes[0]["child"][a] >= 0 and bool(t.nodes[t.nodes[0]["child"][a]].get("marked"))
                    for t, a in zip(pair.trees, actions)]
            pair.reroot(actions, s2)
            value, _ = pair.host.proof()
            status = pair.host.status
            for i, t in enumerate(pair.trees):
                if onto[i]:  # reopened, handed out for evaluation, and proven at once from its kept children
                    assert status[i, 0] == 0 and value[i] != U.UNPROVEN and not t.nodes[0]["pos"].done
                if len(t.nodes) == 1:
                    assert value[i] == U.UNPROVEN  # a fresh root
            res = pair.round()
            for i, t in enumerate(pair.trees):
                if onto[i]:  # rule 5: the proven root got its evaluation and began no descent
                    assert pair.calls >= 1 and t.done == 0
        for k, v in pair.seen().items():
            if k in ("onto", "deeper", "at_once"):
                seen[k] += v
        pair.close()


def test_the_coverage_conditions_hold_on_the_restatement_alone(libs):
    """Needs the two tests above (it runs them for a game whose tally is missing)."""
    for fam in U.GAMES:
        if fam not in _seen or not _seen[fam].get("at_once"):
            for wide in (False, True):
                test_harness_equals_the_restatement_and_every_proof_is_true(libs, fam, wide, "stand_in")
                test_reroot_onto_marked_nodes_keeps_marks_and_proves_the_new_root_at_once(libs, fam, wide)
        seen = _seen[fam]
        want = [k for k in U.EVENTS if k != "draw" or fam in ("TicTacToe", "Othello")]
        missing = [k for k in want if not seen[k]]
        assert not missing, (fam, missing, seen)


# ---- without the flag: today's session ------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", U.GAMES)
def test_flags_0_equals_the_existing_harnesses_byte_for_byte(libs, fam):
    game, roots, _ = roots_of(libs, fam)
    S = U.SIMS[fam]
    for W, D in ((1, 0), (WIDE, 0), (WIDE, 2)):
        off = U.ProveHost(libs, fam, roots, S, W, D, flags=0)
        old = T.TacticsHost(libs, fam, roots, S, W, D) if D else T.TacticsHost(libs, fam, roots, S, W, 0, plain=True)
        guided = None
        if (W, D) == (1, 0):
            guided = plain.HostSession((None, libs["guided"]), f"{fam}-v1", roots, S, U.C_PUCT)
        for t in range(S + 1):
            got, ref = off.leaves(), old.leaves()
            for x, y in zip(got, ref):
                assert np.array_equal(x, y), (fam, W, t)
            priors, values = T.stand_in_rows(got[0], got[1])
            assert off.advance(priors, values) == 0 and old.advance(priors, values) == 0
            for x, y in zip(off.result(), old.result()):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (fam, W, t)
            if guided is not None:
                for x, y in zip(got, guided.leaves()):
                    assert np.array_equal(x[:, 0], y), (fam, t)
                assert guided.advance(priors[:, 0], values[:, 0]) == 0
                for x, y in zip(off.result()[:4], guided.result()):
                    assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (fam, t)
            value, q = off.proof()
            assert (value == U.UNPROVEN).all() and (q == U.UNPROVEN).all()  # nothing is proven without the flag
        if D:
            assert np.array_equal(off.decided()[0], old.decided()[0])
        off.close()
        old.close()
        if guided is not None:
            guided.close()


def test_prove_changes_a_pick_and_a_result_against_the_session_without_it(libs):
    """The same roots and rows with and without the flag: some root's visits differ (rules 4 and 5), and where the
    session without the flag plays a move that is proven to lose, the session with it does not."""
    fam = "ConnectFour"
    game, roots, truth = roots_of(libs, fam)
    S = U.SIMS[fam]
    on, off = U.ProveHost(libs, fam, roots, S, 1, 2), U.ProveHost(libs, fam, roots, S, 1, 2, flags=0)
    for h in (on, off):
        for t in range(S + 1):
            obs, mask, _ = h.leaves()
            assert h.advance(*T.stand_in_rows(obs, mask)) == 0
    (v1, _, a1, _, _), (v0, _, a0, _, _) = on.result(), off.result()
    assert not np.array_equal(v1, v0)
    for i, t in enumerate(truth):
        if t is not None and (t[1][roots[i].mask] != -1).any() and on.proof()[0][i] != U.UNPROVEN:
            assert t[1][a1[i]] == t[0]  # the proven session plays a best move
    on.close()
    off.close()


# ---- the stand-alone program under the host sanitizers --------------------------------------------------------------
def test_the_stand_alone_program_runs_clean_under_the_host_sanitizers(libs):
    exe = U.compile_harness(libs["tmp"], "pgx_prove_host.cpp", shared=False,
                            flags=("-DPGX_PROVE_MAIN", "-g", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=undefined"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 24 and "ERROR" not in out.stderr and "runtime error" not in out.stderr
    assert any("proof -128" not in ln for ln in lines)  # the rounds proved something


# ---- the header's values, the C ABI, the Python layers --------------------------------------------------------------
def test_limits_and_symbols(libs):
    from envpool_amd.core import native

    lim = libs["tactics"].pgx_prove_limits
    assert (lim(0), lim(1)) == (native.GUIDED_PROVE, native.GUIDED_UNPROVEN) == (1, -128)
    header = open(os.path.join(T.ROOT, "include", "envpool_amd.h")).read()
    for name in ("epa_guided_begin_prove", "epa_guided_begin_prove_device", "epa_guided_proof",
                 "epa_guided_proof_device"):
        assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header
    assert "#define EPA_GUIDED_PROVE 1" in header and "#define EPA_GUIDED_UNPROVEN (-128)" in header
    _, roots, _ = roots_of(libs, "TicTacToe")
    for flags in (2, 3, -1):
        U.ProveHost(libs, "TicTacToe", roots[:1], 4, 1, 0, flags=flags, want_rc=-6)


def test_check_guided_prove():
    from envpool_amd.core import native

    assert native.check_guided_prove(None) is False and native.check_guided_prove(False) is False
    assert native.check_guided_prove(True) is True and native.check_guided_prove(np.bool_(True)) is True
    for bad in (1, 0, "yes", 1.0):
        with pytest.raises(ValueError, match="guided_begin: prove = "):
            native.check_guided_prove(bad)


class _Recorder(plain._Recorder):
    def guided_begin(self, env_ids, simulations, c_puct, *more):
        out = super().guided_begin(env_ids, simulations, c_puct)
        if more:
            self.calls[-1] += more
        return out

    def guided_proof(self):
        self.calls.append(("proof",))
        return np.full(self.k, -128, np.int8), np.full((self.k, 65), -128, np.int8)


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool
    from envpool_amd.python.envpool import Proof

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    for bad in (1, "no", 2.0):
        with pytest.raises(ValueError, match="guided_begin: prove = "):
            env.guided_search(ids, simulations=8, prove=bad)
    with pytest.raises(ValueError, match="prove is an argument of policy='puct'"):
        env.guided_search(ids, simulations=8, policy="gumbel", prove=True)
    with pytest.raises(ValueError, match="gumbel_search: prove"):
        env.gumbel_search(ids, simulations=8, prove=True)
    assert env._pool.calls == []
    # the default is today's calls
    gs = env.guided_search(ids, simulations=3, c_puct=0.5, prove=False)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5)] and gs.prove is False
    gs.close()
    env._pool.calls.clear()
    gs = env.guided_search(ids, simulations=3, c_puct=0.5, prove=True)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5, 0, None, 0, 4096, True)] and gs.prove is True
    proof = gs.proof
    assert isinstance(proof, Proof) and proof.value.tolist() == [-128] * 3 and env._pool.calls[-1] == ("proof",)
    gs.close()
    with pytest.raises(ValueError, match="closed"):
        gs.proof
    env._pool.calls.clear()
    gs = env.guided_search(ids, simulations=3, c_puct=0.5, nodes=9, width=4, tactics=2, tactics_nodes=64, prove=True)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5, 9, 4, 2, 64, True)] and gs.width == 4
    gs.close()
