"""Generate golden rollouts from the REFERENCE ITSELF (oracle/_ref = the
reference's C++ compiled in place from /root/reference; see oracle/Makefile).

Run in the build container only (needs /root/reference):
    make -C oracle ref && python tests/golden/make_golden.py
Writes tests/golden/<task_id>.npz, for every case that has no file yet (a file that exists is left
untouched: delete it to have it made again), holding the seeded action sequence and every
state key the reference returned for reset + T steps (auto-resets included).
The reference has no golden vectors of its own for these envs, so
these files are the pin for oracle/restate and for the HIP engine.

The Blackjack natural / sab cases assert what they are there for before they are written: a 1.5 reward
with natural and without sab, none otherwise, and without either rule a stick on a natural that pays 1.0.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.orc import Oracle  # noqa: E402
from oracle_cases import CASES, sample_actions  # noqa: E402

N, T, SEED = 8, 400, 42


def check_blackjack(name, extra, out) -> None:
    """The reward branches of blackjack.h:85-99 that the case is about."""
    natural, sab = extra
    rew = out["state/reward"].reshape(T + 1, N)
    obs = out["state/obs"].reshape(T + 1, N, 3)
    first = out["state/elapsed_step"].reshape(T + 1, N)[:-1] == 0
    # a natural: 21 with a usable ace on the two cards of the reset; then a stick
    stick_on_natural = first & (obs[:-1, :, 0] == 21) & (obs[:-1, :, 2] == 1) & (out["actions"] == 0)
    assert stick_on_natural.any(), (name, "no stick on a natural")
    assert ((rew == 1.5).any()) == bool(natural and not sab), (name, "1.5 rewards")
    paid = rew[1:][stick_on_natural]
    if natural and not sab:
        assert (paid == 1.5).any(), name
    elif not sab:
        assert (paid == 1.0).any() and set(paid.tolist()) <= {0.0, 1.0}, name
    print(name, "sticks on a natural:", int(stick_on_natural.sum()), "rewards", sorted(set(paid.tolist())))


def main() -> None:
    for name, c in CASES.items():
        path = os.path.join(HERE, name + ".npz")
        if os.path.exists(path):
            continue
        o = Oracle(c["task"], N, seed=SEED, max_episode_steps=c["max_steps"],
                   extra=c["extra"], kind="reference", num_threads=2)
        rng = np.random.default_rng(1234)
        frames = [o.reset()]
        actions = []
        for _ in range(T):
            a = sample_actions(c, rng, N)
            actions.append(a)
            frames.append(o.step(a))
        out = {"actions": np.stack(actions), "seed": np.int64(SEED)}
        for k in frames[0]:
            out["state/" + k] = np.stack([f[k] for f in frames])
        if c["task"] == "Blackjack":
            check_blackjack(name, c["extra"], out)
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
