"""Shared by the training tests of the memory actor (test_actor_memory_train_host.py, test_gpu_actor_memory_train.py):
the cases, the reference -- the float64 twin `Actor.module().unroll` with autograd --, and ONE numpy restatement of the
same backward pass through time (csrc/actor_memory_train.hip.h) that can also run over magnitudes: the G_abs of the
error bound."""
import numpy as np
import torch

from actor_memory_util import rs
from envpool_amd.actor import Actor
from pgx_train_util import forward_np

NAMES = ("Wz", "Wn", "bz", "bn", "dh0")


def case(f, m, n, t, kind, seed=0):
    """(actor, obs float64 [T, N, F] whose features are its own integers, h0 uint8 [N, M], mask bool [T, N] with
    consecutive zeros, a zero at t = 0 and one at t = T - 1, g: the loss's weights of logits, value and h)."""
    rng = np.random.default_rng([f, m, n, t, kind, seed])
    spec = dict(features=f, kind=kind, actions=3, low=-np.ones(3 * kind, np.float32), high=np.ones(3 * kind, np.float32),
                obs_low=np.zeros(f), obs_high=np.full(f, 127.0))
    a = Actor.random(spec, hidden=32, blocks=1, seed=seed, memory=m)
    # (shifts 2 below Actor.random's: the sums spread over four times the range, so every regime of both clamps is met)
    actor = Actor(a.net, kind, a.lo, a.scale, a.sigma, a.low, a.high, cell=[(w, b, s - 2) for w, b, s in a.cell])
    obs = rng.integers(0, 128, (t, n, f)).astype(np.float64)
    h0 = rng.integers(0, 128, (n, m)).astype(np.uint8)
    mask = rng.random((t, n)) < 0.7
    mask[0, 0] = mask[t - 1, 1] = mask[t // 2, 2] = mask[max(t // 2 - 1, 0), 2] = False
    g = (rng.standard_normal((t, n, 3)).astype(np.float32), rng.standard_normal((t, n)).astype(np.float32),
         rng.standard_normal((n, m)))
    return actor, obs, h0, mask, g


def twin(actor, obs, h0, mask, g, kernels=False, device="cpu"):
    """((logits, value, h), grads) of the module for the loss SUM logits gl + SUM value gv + SUM h gh: torch tensors on
    the CPU and a dict of float64 numpy -- NAMES and ("w", i), ("b", i) of the trunk."""
    mod = actor.module().to(device)
    h0 = torch.tensor(h0.astype(np.float64), device=device, requires_grad=True)
    args = (torch.tensor(obs, device=device), h0, torch.tensor(mask, device=device))
    out = mod.unroll(*args, kernels=True) if kernels else mod.unroll(*args)
    sum((o * torch.tensor(w, device=device)).sum() for o, w in zip(out, g)).backward()
    grads = dict(zip(NAMES, (*mod.cell_weights, *mod.cell_biases, h0)))
    grads.update({("w", i): w for i, w in enumerate(mod.net.weights)})
    grads.update({("b", i): b for i, b in enumerate(mod.net.biases)})
    return tuple(o.detach().cpu() for o in out), {k: v.grad.cpu().numpy().astype(np.float64) for k, v in grads.items()}


def forward_np_cell(actor, obs, h0, mask):
    """Per step (h_in, pre_z, pre_n, h'), all int64 [N, M]: the values before the two clamps."""
    (wz, bz, sz), (wn, bn, sn) = [(w.astype(np.int64), b.astype(np.int64), s) for w, b, s in actor.cell]
    h, steps = h0.astype(np.int64), []
    for t in range(len(obs)):
        v = np.concatenate([obs[t].astype(np.int64), h], axis=1)
        pre_z, pre_n = 64 + rs(v @ wz.T + bz, sz), rs(v @ wn.T + bn, sn)
        z, n = np.clip(pre_z, 0, 128), np.clip(pre_n, 0, 127)
        steps.append((h, pre_z, pre_n, (z * h + (128 - z) * n + 64) >> 7))
        h = steps[-1][3] * mask[t][:, None]
    return steps


def backward_np(actor, obs, h0, mask, g, absolute=False):
    """`twin`'s grads by the contract's rules in float64.  `absolute`: over |W|, the magnitudes of the incoming
    gradients and of the local factors (|h - n|, 128 - z, z) with the same masks."""
    mag = np.abs if absolute else (lambda a: a)
    net, f = actor.net, obs.shape[2]
    t_n = obs.shape[0] * obs.shape[1]
    steps = forward_np_cell(actor, obs, h0, mask)
    hp = np.concatenate([s[3] for s in steps])
    out = {}
    # the trunk, all slots at once: pgx_train.hip.h's rules, and one more product for its input
    pre, _ = forward_np(net, hp)
    act = [hp.astype(np.float64)] + [np.clip(q, 0, 127).astype(np.float64) for q in pre]
    keep = [None] + [((q >= 0) & (q <= 127)).astype(np.float64) for q in pre]
    wt = [mag(w.astype(np.float64)) for w, _, _ in net.layers]
    sc = [2.0 ** -s for _, _, s in net.layers]
    dp = np.concatenate([g[0] * np.float32(net.scale_p), (g[1] * np.float32(net.scale_v))[:, :, None]], axis=2)
    dz, res = mag(dp.reshape(t_n, -1).astype(np.float64)), None
    for i in range(len(net.layers) - 1, -1, -1):
        out["w", i], out["b", i] = dz.T @ act[i], dz.sum(axis=0)
        dx = dz @ wt[i]
        if i == 0:
            break
        if i % 2 == 0:                     # below a block's second layer: remember the gradient of h_new
            res = dz / sc[i]
        elif i < len(net.layers) - 1:      # below its first layer: the residual branch joins
            dx = dx + res
        dz = dx * keep[i] * sc[i - 1]
    dhp = dx.reshape(obs.shape[0], obs.shape[1], -1)
    # the cell, backward through time
    (wz, _, sz), (wn, _, sn) = actor.cell
    wz, wn = mag(wz.astype(np.float64)), mag(wn.astype(np.float64))
    carry = mag(g[2].astype(np.float64))
    out.update(Wz=0.0, Wn=0.0, bz=0.0, bn=0.0)
    for t in range(len(obs) - 1, -1, -1):
        h, pre_z, pre_n, _ = steps[t]
        z, n = np.clip(pre_z, 0, 128), np.clip(pre_n, 0, 127)
        dy = dhp[t] + carry * mask[t][:, None]
        da_z = dy * mag((h - n) / 128.0) * ((pre_z >= 0) & (pre_z <= 128)) * 2.0 ** -sz
        da_n = dy * (128 - z) / 128.0 * ((pre_n >= 0) & (pre_n <= 127)) * 2.0 ** -sn
        v = np.concatenate([obs[t], h.astype(np.float64)], axis=1)
        out["Wz"], out["Wn"] = out["Wz"] + da_z.T @ v, out["Wn"] + da_n.T @ v
        out["bz"], out["bn"] = out["bz"] + da_z.sum(axis=0), out["bn"] + da_n.sum(axis=0)
        carry = dy * z / 128.0 + da_z @ wz[:, f:] + da_n @ wn[:, f:]
    out["dh0"] = carry
    return out


def regimes(actor, obs, h0, mask):
    """The least share of the elements that any of the six regimes holds: the gate below 0, inside, above 128; the
    candidate below 0, inside, above 127."""
    steps = forward_np_cell(actor, obs, h0, mask)
    pre_z, pre_n = np.stack([s[1] for s in steps]), np.stack([s[2] for s in steps])
    return min(np.mean(q) for q in (pre_z < 0, (pre_z >= 0) & (pre_z <= 128), pre_z > 128,
                                    pre_n < 0, (pre_n >= 0) & (pre_n <= 127), pre_n > 127))
