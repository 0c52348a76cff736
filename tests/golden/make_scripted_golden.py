"""Generate the scripted golden rollouts from the REFERENCE ITSELF (oracle/_ref = the reference's C++ compiled
in place; see oracle/Makefile), closed loop: the policies of tests/scripted_cases.py look at the reference's own
observations and steer it into the branches that the random rollouts of make_golden.py never take.

Run where the reference is:
    make -C oracle ref && python tests/golden/make_scripted_golden.py
Writes tests/golden/scripted_<case>.npz for every case that has no file yet (a file that exists is left untouched:
delete it to have it made again), in the layout of make_golden.py's files: the actions the policy chose, the seed,
and every state key the reference returned for reset + T steps.  A replay is open loop from the recorded actions.

Every case asserts the events it exists for (scripted_cases.SCRIPTED[...]["events"]) before its file is written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.orc import Oracle  # noqa: E402
from scripted_cases import N, SCRIPTED, SEED, check_events, rollout  # noqa: E402


def main() -> None:
    for name, c in SCRIPTED.items():
        path = os.path.join(HERE, "scripted_" + name + ".npz")
        if os.path.exists(path):
            continue
        assert c["T"] <= 500
        o = Oracle(c["task"], N, seed=SEED, max_episode_steps=c["max_steps"], extra=c["extra"], kind="reference",
                   num_threads=2)
        out = rollout(o, c, N)
        out["seed"] = np.int64(SEED)
        print(name, check_events(name, out))
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
