"""Training kernels of the memory actor on the device (csrc/actor_memory_train.hip.h): `unroll(..., kernels=True)` on a
ROCm device against the float64 twin on the CPU.  The forward is equal; every gradient is within
depth * kCellTrainErr * G_abs, G_abs from the restatement's pass over magnitudes; a second run gives the same bits.
(F, M): F off a multiple of 4 with one column tile, and three column tiles over four waves; N: a ragged tile and more
than one block; the last case has two column tiles per wave and tiles of 64 rows (N >= 16384) in both kernels."""
import numpy as np
import pytest
import torch

import actor_memory_train_util as tu
from envpool_amd import actor_memory_train as amt

pytestmark = pytest.mark.gpu

CASES = [(f, m, n, t, kind) for f, m in ((19, 32), (5, 96)) for n in (37, 70) for t in (1, 5) for kind in (0, 1)]
CASES.append((7, 160, 16389, 2, 0))


@pytest.mark.parametrize("f,m,n,t,kind", CASES)
def test_unroll_kernels_against_the_twin(f, m, n, t, kind):
    c = tu.case(f, m, n, t, kind)
    actor = c[0]
    assert tu.regimes(*c[:4]) >= 0.02, "the inputs must exercise every regime of both clamps"
    want, want_g = tu.twin(*c)
    got, got_g = tu.twin(*c, kernels=True, device="cuda")
    for a, b, name in zip(got, want, ("logits", "value", "h")):
        assert torch.equal(a, b), name
    top = tu.backward_np(*c, absolute=True)
    layers = len(actor.net.layers)
    for k in want_g:
        depth = layers - k[1] if isinstance(k, tuple) else amt.depth(actor.net.blocks, t)
        err, bound = np.abs(got_g[k] - want_g[k]), depth * amt.ERR * top[k]
        print(f"{k}: largest error / bound = {np.max(err / np.maximum(bound, 1e-300)):.4f}")
        assert (err <= bound).all(), k
    again, again_g = tu.twin(*c, kernels=True, device="cuda")
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    assert all(np.array_equal(again_g[k], got_g[k]) for k in got_g)
