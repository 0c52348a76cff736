"""The PGX rules at crafted positions, CPU side.  The scalar restatement of the rules (pgx_rules_ref.py) replays
every reference fixture bit for bit, which pins it to the reference; the g++ build of the kernel's env code
(envpool_amd/csrc/pgx_env.hip.h through tests/cpu_harness/pgx_host.cpp: SetHidden, Step, Elem, Hidden -- the path of
set_state, send, recv and get_state) then has to agree with it on every key and the hidden words, with no tolerance,
at the position families of pgx_rules_families.py.  One-token mutants of the header show that the families notice."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pgx_rules_families as F
import pgx_rules_ref as R
from pgx_util import CODE, GOLDEN, IDS, KEYS, NAMES, fixture, game, hidden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join("envpool_amd", "csrc", "pgx_env.hip.h")
HARNESS = os.path.join("tests", "cpu_harness", "pgx_host.cpp")


def build(root, out, opt="-O2"):
    subprocess.run(["g++", opt, "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(root, HARNESS),
                    "-o", out], check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(ROOT, str(tmp_path_factory.mktemp("pgx_rules") / "libpgxhost.so"))


def host_step(lib, name, done=0, expect=0):
    """The family's rows through the harness: every key [n, ...] and the hidden words after the step."""
    fam, want, _ = F.family(name)
    g, n = fam["game"], len(fam["actions"])
    outs = {k: np.zeros_like(want[k]) for k in R.KEYS}
    hid = np.zeros((n, R.hidden_words(g)), np.int32)
    over = np.full(n, done, np.int32)
    ptrs = (ctypes.c_void_p * len(R.KEYS))(*[outs[k].ctypes.data for k in R.KEYS])

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    hidden_in = np.ascontiguousarray(fam["hidden"], np.int32)
    rc = lib.pgx_step_rows(CODE[g], n, p(hidden_in), p(fam["elapsed"]), p(over), p(fam["actions"]),
                           int(fam["limit"]), ptrs, p(hid))
    assert rc == expect, rc
    return outs, hid


def test_restatement_names_the_engines_keys():
    assert R.KEYS == KEYS


@pytest.mark.parametrize("name", NAMES)
def test_restatement_replays_fixture_bit_exact(name):
    g = fixture(name)
    outs, hid = R.replay(game(name), g, hidden(g))
    for k in KEYS:
        assert outs[k].dtype == g[k].dtype and np.array_equal(outs[k], g[k]), (name, k)
    assert np.array_equal(hid, hidden(g)), name


@pytest.mark.parametrize("tid", IDS)
def test_scripted_fixture_holds_the_required_content(tid):
    """The fixtures the reference made from scripted games: every ConnectFour line, Othello's wipe-outs, second
    passes, ties and longest captures, moves onto occupied cells, Hex's swaps and long chains, ... (the generator's
    own check, tests/golden/pgx_scripted.py, on the committed file); short enough for the sweeps over NAMES."""
    sys.path.insert(0, GOLDEN)
    import pgx_scripted

    assert f"{tid}__scripted" in NAMES
    g = fixture(f"{tid}__scripted")
    pgx_scripted.check(game(tid), g)
    assert g["actions"].size <= 4000 and (g["elapsed_step"][1:] == 0).any()


@pytest.mark.parametrize("name", sorted(F.FAMILIES))
def test_host_build_agrees_with_restatement(harness, name):
    outs, hid = host_step(harness, name)
    assert F.differences(name, outs, hid) == [], name


def test_harness_refuses_rows_that_are_over_or_no_state(harness):
    host_step(harness, "hex_swap", done=1, expect=-3)
    fam = F.family("c4_last_cell")[0]
    keep = fam["hidden"][0, 0]
    try:
        fam["hidden"][0, 0] = 2  # no color
        host_step(harness, "c4_last_cell", expect=-2)
    finally:
        fam["hidden"][0, 0] = keep


def test_families_see_every_kind_of_row():
    """Per game: both step types, a truncated and an untruncated ending, both seats to move, every reward pair of
    an ending."""
    for g in R.A:
        names = [n for n in F.FAMILIES if F.family(n)[0]["game"] == g]
        want = {k: np.concatenate([F.family(n)[1][k] for n in names]) for k in R.KEYS}
        assert set(want["step_type"]) == {1, 2}, g
        assert want["trunc"].any() and (want["done"] & ~want["trunc"]).any(), g
        assert set(want["info:current_player"]) == {0, 1}, g
        pairs = {tuple(r) for r in want["reward"][want["done"]]}
        assert {(1.0, -1.0), (-1.0, 1.0)} <= pairs and (g == "Hex" or (0.0, 0.0) in pairs), (g, pairs)
        assert sum(1 for n in names if n in F.TRUNC) == 1, g


# one-token edits of the header: (pattern, replacement); each pattern occurs exactly once
MUTANTS = {
    "c4_d1_mask": ("(b >> 24) & c0_3;", "(b >> 24);"),
    "c4_d2_mask": ("(b >> 18) & c3_6;", "(b >> 18);"),
    "c4_h_mask": ("(b >> 3) & c0_3;", "(b >> 3);"),
    "c4_filled_bound": ("cell = filled < 6 ?", "cell = filled < 5 ?"),
    "othello_moves_count": ("for (int i = 0; i < 5; ++i) t |=", "for (int i = 0; i < 4; ++i) t |="),
    "othello_shift_edge": ("case 4: return (x & not_c0) << 7;", "case 4: return (x & not_c7) << 7;"),
    "othello_wiped": ("wiped = opp == 0;", "wiped = my == 0;"),
    "hex_col0": ("const u128 ym = f & ~col0,", "const u128 ym = f,"),
    "hex_diagonal": ("| (yp >> 10);", "| (yp >> 12);"),
    "hex_edge_parity": ("if ((s.turn & 1) == 0) {", "if ((s.turn & 1) != 0) {"),
    "hex_swap_transpose": ("const int sw = (ix % 11) * 11 + ix / 11;", "const int sw = (ix / 11) * 11 + ix % 11;"),
}


def test_rule_tests_catch_mutants(tmp_path):
    """Each mutant of the header, built into the harness, differs from the restatement in some family.  (CPU only:
    mutants are never built for a GPU.)"""
    text = open(os.path.join(ROOT, HEADER)).read()
    order = sorted(F.FAMILIES, key=lambda n: len(F.family(n)[0]["actions"]))
    missed = []
    for tag, (old, new) in MUTANTS.items():
        assert len(re.findall(re.escape(old), text)) == 1, tag
        root = tmp_path / tag
        os.makedirs(root / os.path.dirname(HEADER))
        os.makedirs(root / os.path.dirname(HARNESS))
        (root / HEADER).write_text(text.replace(old, new))
        shutil.copy(os.path.join(ROOT, HARNESS), root / HARNESS)
        lib = build(str(root), str(root / "libmutant.so"), opt="-O1")
        caught = None
        for name in order:
            outs, hid = host_step(lib, name)
            if F.differences(name, outs, hid):
                caught = name
                break
        print(f"mutant {tag}: caught by {caught}")
        if caught is None:
            missed.append(tag)
    assert missed == []
