"""Training kernels of the memory actor, what needs no device: `unroll(..., kernels=True)` on CPU tensors is the twin's
code, the C ABI's new names, the refusals that stay, and the numpy restatement of the backward through time
(actor_memory_train_util) against the twin's autograd."""
import numpy as np
import pytest
import torch

import actor_memory_train_util as tu
from envpool_amd.core import native

NEW = ["epa_cell_train_create", "epa_cell_train_destroy", "epa_cell_train_forward_device",
       "epa_cell_train_backward_device", "epa_net_train_input_grad_device"]


@pytest.mark.parametrize("kind", [0, 1])
def test_kernels_on_cpu_tensors_is_the_twin(kind):
    c = tu.case(19, 32, 37, 5, kind)
    want, want_g = tu.twin(*c)
    got, got_g = tu.twin(*c, kernels=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(got_g[k], want_g[k]) for k in want_g)
    mod = c[0].module()
    with pytest.raises(ValueError, match="require grad"):
        mod.unroll(torch.tensor(c[1], requires_grad=True), torch.tensor(c[2]), torch.tensor(c[3]), kernels=True)


def test_names_and_refusals():
    header = open("include/envpool_amd.h").read()
    sig = native.lib()
    for name in NEW:
        assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header and hasattr(sig, name), name
    actor = tu.case(5, 32, 3, 1, 0)[0]
    for refused in (actor.trainer, lambda: actor.module(kernels=True)):
        with pytest.raises(ValueError, match="memory actor"):
            refused()


@pytest.mark.parametrize("f,m,n,t,kind", [(19, 32, 37, 5, 0), (5, 96, 70, 5, 1), (5, 96, 37, 1, 0)])
def test_restatement_equals_autograd(f, m, n, t, kind):
    c = tu.case(f, m, n, t, kind)
    assert tu.regimes(*c[:4]) >= 0.02
    _, want = tu.twin(*c)
    got, top = tu.backward_np(*c), tu.backward_np(*c, absolute=True)
    for k in want:
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
        assert (np.abs(got[k]) <= top[k] * (1 + 1e-12)).all(), k
