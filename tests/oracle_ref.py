"""The oracle's side of a persistent launch (test infrastructure): consecutive episodes of one env, the launch model with budgets
and restarts, summary rows, and the rollout log against the oracle's lists.  No test module defines these for itself."""
import ctypes as C

import numpy as np


def opol(name):
    import oracle
    return {"random": oracle.POLICY_RANDOM, "first": oracle.POLICY_FIRST, "nearest": oracle.POLICY_NEAREST}[name]


def one(inst, b, t=None):
    """Env b's slice of a batch, cut to the env's own t tasks."""
    return dict(depot=inst["depot"][b], task_xy=inst["task_xy"][b, :t], req=inst["req"][b, :t], dur=inst["dur"][b, :t])


def episodes(a, t, inst_one, seed, policy, n, mwt=10.0, record=False, d0=0, max_time=100.0):
    """n consecutive oracle episodes of one env, the decision counter running on across them from d0.  inst_one: the env's instance, or
    a callable k -> the instance of episode k; where that returns (A_k, instance), episode k has that instance's own sizes."""
    import oracle
    oracle.build()
    out = []
    for k in range(n):
        i = inst_one(k) if callable(inst_one) else inst_one
        ak, tk = a, t
        if isinstance(i, tuple):
            ak, i = i
            tk = i["req"].shape[0]
        r = oracle.OracleEnv(ak, tk, max_waiting_time=mwt, max_time=max_time).load(i["depot"], i["task_xy"], i["req"], i["dur"]) \
            .rollout(int(seed), d0, opol(policy), cap_steps=20000, record=record)
        out.append(r)
        d0 += r["n_steps"]
    return out


def episodes_first_recorded(a, t, inst_one, seed, policy, n, mwt=10.0, max_time=100.0):
    """episodes() on one instance with the first episode's decisions recorded and the later ones' not."""
    first = episodes(a, t, inst_one, seed, policy, 1, mwt, record=True, max_time=max_time)
    return first + episodes(a, t, inst_one, seed, policy, n - 1, mwt, d0=first[0]["n_steps"], max_time=max_time)


def two_episodes(inst, seeds, a, t, mwt=10.0, max_time=100.0):
    """(first-episode traces, second-episode results) of every env of a batch under the random policy, at the envs' sizes (a, t)."""
    eps = [episodes_first_recorded(a, t, one(inst, b, t), seeds[b], "random", 2, mwt, max_time) for b in range(len(seeds))]
    return [e[0] for e in eps], [e[1] for e in eps]


def summary_row(r):
    """The row dcm_summary holds after the episode r."""
    return np.array([r["reward"], float(r["finished"].sum()), *r["metrics"][:6]], np.float64)


def assert_summary(sm, ref, name):
    assert sm[0] == ref["reward"] and int(sm[1]) == int(ref["finished"].sum()), f"{name}: reward / finished tasks"
    for i in range(6):
        assert sm[2 + i] == ref["metrics"][i], f"{name}: metric {i} {sm[2 + i]!r} != {ref['metrics'][i]!r}"


def play(a, t, one, seed, d0, policy, cap, mwt, max_time=100.0):
    """One oracle episode of at most `cap` decisions (None: to its end) from decision counter d0.  Returns (the OracleEnv, whose
    route() lists are those of the decisions taken; decisions taken; whether the episode ended).  The raw return value tells a cap
    that cut the episode (-1) from an episode of exactly `cap` decisions."""
    import oracle
    o = oracle.OracleEnv(a, t, max_waiting_time=mwt, max_time=max_time).load(one["depot"], one["task_xy"], one["req"], one["dur"])
    n = oracle.lib().orc_rollout(o._h, C.c_uint64(int(seed)), C.c_uint64(int(d0)), opol(policy), 1 << 40 if cap is None else int(cap),
                                 *([None] * 12))
    return (o, int(cap), False) if n < 0 else (o, int(n), True)


class Sim:
    """What the persistent kernels do with one env over a sequence of launches, in oracle episodes: an env that is in the middle of an
    episode plays it to its end (one of the launch's `episodes`), a finished env restarts -- on instance inst_of(j) for its j-th
    restart -- unless its budget is spent, and a spent budget stops it where it is.  `.o` is the OracleEnv of the episode the log
    should hold."""

    def __init__(self, a, t, inst_of, seed, policy, mwt=10.0, max_time=100.0):
        self.a, self.t, self.inst_of, self.seed, self.policy, self.mwt, self.max_time = a, t, inst_of, seed, policy, mwt, max_time
        self.j, self.d0, self.k, self.done, self.o = 0, 0, 0, False, None

    def launch(self, episodes, budget):
        left = None if budget < 0 else int(budget)
        if self.policy != "random" and not self.mwt > 0.0 and left is None:
            left = 0                                            # a greedy "no limit" on a max_waiting_time <= 0 handle counts as 0
        taken = 0
        for _ in range(episodes):
            if self.done:
                if left == 0:
                    break
                self.j, self.d0, self.k, self.done = self.j + 1, self.d0 + self.k, 0, False
            elif left == 0:
                break
            o, k, ended = play(self.a, self.t, self.inst_of(self.j), self.seed, self.d0, self.policy,
                               None if left is None else self.k + left, self.mwt, self.max_time)
            taken += k - self.k
            if left is not None:
                left -= k - self.k
            self.o, self.k, self.done = o, k, ended
            if left == 0:
                break
        return taken


def log(env):
    return tuple(x.cpu().numpy() for x in env.rollout_routes())


def assert_log(log, b, sim, tag):
    """Env b's rows against the oracle episode they should hold (sim: .o and .a): the true lengths, the stored prefix of every list,
    nothing written behind it, and nothing in the rows of agents the env does not have."""
    task, arr, ln = log
    cap = task.shape[2]
    for a in range(task.shape[1]):
        rt, ra = sim.o.route(a) if (a < sim.a and sim.o is not None) else (np.zeros(0, np.int32), np.zeros(0))
        n = min(len(rt), cap)
        assert ln[b, a] == len(rt), f"{tag} env{b} agent{a}: length {ln[b, a]} != {len(rt)}"
        assert np.array_equal(task[b, a, :n], rt[:n].astype(np.int16)), f"{tag} env{b} agent{a}: route"
        assert np.array_equal(arr[b, a, :n].view(np.uint64), ra[:n].view(np.uint64)), f"{tag} env{b} agent{a}: arrival times"
        if a >= sim.a:
            assert (task[b, a] == -2).all() and (arr[b, a] == 0.0).all(), f"{tag} env{b}: row of agent {a} beyond the env's size"
