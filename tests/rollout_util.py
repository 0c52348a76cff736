"""The rollout collector's contract (envpool_amd/csrc/rollout.hip.h, DESIGN.md section 2 "Rollout collector") restated
in numpy.  `Model` is fed what a plain pool's `recv` returned -- a dict by state key, rows in any order -- and the
action rows that were sent; float32 and float64 arithmetic is done element by element in the contract's order (numpy
rounds every elementwise operation on its own: nothing is fused)."""
import numpy as np

LEAF, LEAVES = 16, 16  # rollout.hip.h: kMomentLeaf, kMomentLeaves


def tree_sums(x):
    """(sum, sum of squares) of the rows of x [N, C] by the contract's tree, per component, float64."""
    x = np.asarray(x).reshape(len(x), -1).astype(np.float64)
    n, c = x.shape
    s1, s2 = np.zeros(c), np.zeros(c)
    for g0 in range(0, n, LEAF * LEAVES):
        t1, t2 = np.zeros(c), np.zeros(c)
        for l0 in range(g0, g0 + LEAF * LEAVES, LEAF):
            a, b = np.zeros(c), np.zeros(c)
            for r in range(min(l0, n), min(l0 + LEAF, n)):
                a = a + x[r]
                b = b + x[r] * x[r]
            t1, t2 = t1 + a, t2 + b
        s1, s2 = s1 + t1, s2 + t2
    return s1, s2


def gae(reward, term, trunc, mask, values, gamma, lam):
    """(adv, ret) float32 [T, N]: the contract's recurrence, every operation in float32, flags by selection."""
    reward, values = np.asarray(reward, np.float32), np.asarray(values, np.float32)
    gamma, lam = np.float32(gamma), np.float32(lam)
    gl = np.float32(gamma * lam)
    t_max, n = reward.shape
    adv, ret = np.zeros((t_max, n), np.float32), np.zeros((t_max, n), np.float32)
    nxt = np.zeros(n, np.float32)
    for t in range(t_max - 1, -1, -1):
        boot = (reward[t] + (gamma * values[t + 1]).astype(np.float32)).astype(np.float32)
        d = np.where(term[t] != 0, reward[t], boot)
        delta = (d - values[t]).astype(np.float32)
        cont = (delta + (gl * nxt).astype(np.float32)).astype(np.float32)
        a = np.where((term[t] != 0) | (trunc[t] != 0), delta, cont)
        a = np.where(mask[t] != 0, a, np.float32(0)).astype(np.float32)
        adv[t], ret[t], nxt = a, (a + values[t]).astype(np.float32), a
    return adv, ret


class Model:
    def __init__(self, n, horizon, capacity, obs_keys, id_offset=0, moments=False):
        """obs_keys: the state key names the collector stores (those that start with "obs"), in key order."""
        self.n, self.T, self.cap, self.off, self.names = n, horizon, capacity, id_offset, list(obs_keys)
        self.moments_on = moments
        self.t, self.steps = 0, 0
        self.obs = None
        self.carry = np.zeros(n, bool)
        self.acc_ret, self.acc_len = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self.eps = []  # (env_id, step, ret, length)
        self.finished = self.dropped = 0
        self.mom = None

    def _rows(self, state):
        e = np.asarray(state["info:env_id"]).astype(np.int64) - self.off
        assert sorted(e.tolist()) == list(range(self.n))
        return e

    def _store_obs(self, state, e, slot):
        if self.obs is None:
            self.obs = {k: np.zeros((self.T + 1, *np.asarray(state[k]).shape), np.asarray(state[k]).dtype)
                        for k in self.names}
        for k in self.names:
            self.obs[k][slot][e] = state[k]
        if self.moments_on:
            parts = [tree_sums(self.obs[k][slot]) for k in self.names if self.obs[k].dtype.kind == "f"]
            s1 = np.concatenate([p[0] for p in parts])
            s2 = np.concatenate([p[1] for p in parts])
            if self.mom is None:
                self.mom = np.zeros((3, len(s1)))
            self.mom[0] = self.mom[0] + float(self.n)
            self.mom[1] = self.mom[1] + s1
            self.mom[2] = self.mom[2] + s2

    def reset(self, state):
        self.t = 0
        self._store_obs(state, self._rows(state), 0)
        self.carry[:] = False
        self.acc_ret[:] = 0
        self.acc_len[:] = 0

    def step(self, action, state):
        """action: the rows sent, row i being the action of the env of the batch's row i."""
        assert self.t < self.T
        e, t = self._rows(state), self.t
        if t == 0 and not hasattr(self, "action"):
            a = np.asarray(action)
            self.action = np.zeros((self.T, *a.shape), a.dtype)
            self.reward = np.zeros((self.T, self.n), np.float32)
            self.term, self.trunc, self.mask = (np.zeros((self.T, self.n), np.uint8) for _ in range(3))
        self._store_obs(state, e, t + 1)
        self.action[t][e] = action
        done, trunc, rew = (np.zeros(self.n, bool), np.zeros(self.n, bool), np.zeros(self.n, np.float32))
        done[e] = np.asarray(state["done"]).reshape(-1) != 0
        trunc[e] = np.asarray(state["trunc"]).reshape(-1) != 0
        rew[e] = np.asarray(state["reward"], np.float32).reshape(-1)
        mask = ~self.carry
        self.reward[t], self.mask[t] = rew, mask
        self.term[t], self.trunc[t] = done & ~trunc, trunc
        self.carry = done.copy()
        self.acc_ret = np.where(mask, self.acc_ret + rew.astype(np.float64), self.acc_ret)
        self.acc_len = np.where(mask, self.acc_len + 1, self.acc_len).astype(np.int32)
        for env in np.flatnonzero(done):  # env id order
            self.finished += 1
            if len(self.eps) < self.cap:
                self.eps.append((int(env) + self.off, self.steps, float(self.acc_ret[env]), int(self.acc_len[env])))
            else:
                self.dropped += 1
        self.acc_ret[done] = 0
        self.acc_len[done] = 0
        self.t += 1
        self.steps += 1

    def next(self):
        for k in self.names:
            self.obs[k][0] = self.obs[k][self.t]
        self.t = 0

    def batch(self):
        t = self.t
        return ({k: v[:t + 1] for k, v in self.obs.items()}, self.action[:t], self.reward[:t], self.term[:t],
                self.trunc[:t], self.mask[:t])

    def gae(self, values, gamma, lam):
        assert self.t == self.T
        return gae(self.reward, self.term, self.trunc, self.mask, values, gamma, lam)

    def episodes(self):
        eps, self.eps = self.eps, []
        return (np.array([x[0] for x in eps], np.int32), np.array([x[1] for x in eps], np.int64),
                np.array([x[2] for x in eps], np.float64), np.array([x[3] for x in eps], np.int32))
