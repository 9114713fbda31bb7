"""The device lookahead policy against the oracle (test infrastructure): rollout(policy, lookahead=True) must take, at every decision,
the action with the largest (finished tasks, reward) among the unmasked ones, where an action's value is the result of the episode in
which the decision takes it and the base policy plays every later decision -- Lookahead.values() + best_actions(), restated on the
step-wise oracle walker of lookahead_ref.py.  The cases the CPU and the GPU tests share live here, each computed once."""
import functools

import numpy as np

import lookahead_ref as LA
import oracle_ref as O

GAMMA = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
DONE, FINISHED, TRUNCATED = 1, 2, 4


def shifted_seed(seed, d0):
    """A running decision counter is a seed shift: key_1 = mix64(seed + GAMMA (d + 1)), and every draw of decision d derives from it, so
    the episode that starts at counter d0 under `seed` is the episode that starts at 0 under this seed."""
    return (int(seed) + GAMMA * int(d0)) & MASK64


def lookahead_walk(a, t, inst_one, seed, policy, mwt=10.0, max_time=LA.MAX_TIME):
    """LA.walk with the lookahead rule as action_of.  At decision d every unmasked action a is valued by the oracle's result of
    LA.policy_walk(..., forced={0: a_0, ..., d-1: a_{d-1}, d: a}) -- a_0 .. a_{d-1} the lookahead's own earlier choices -- and the
    largest LA.pair wins, ties to the lowest action (strict > in ascending order).
    Returns the walk's dict plus base_action[n] (what the base policy would have taken at each decision), n_unmasked[n], result (the
    oracle's replay of the walk: LA.result), o (the OracleEnv of that replay, for its route lists) and flags (what the env's header
    holds after the episode: DONE, FINISHED iff check_finished() was true -- every agent returned and every task finished, which is
    only evaluated, and can only hold, when nobody can decide any more -- and TRUNCATED from the oracle's guard)."""
    import oracle
    seed = int(seed)
    chosen, base, nfree = {}, [], []

    def action_of(c):
        best, best_pair = None, None
        for act in np.flatnonzero(c.mask == 0):
            w = LA.policy_walk(a, t, inst_one, seed, policy, mwt, forced={**chosen, c.d: int(act)}, max_time=max_time)
            p = LA.pair(LA.result(a, t, inst_one, w, mwt, max_time))
            if best is None or p > best_pair:
                best, best_pair = int(act), p
        assert best is not None, "the mask always allows an action: the depot when no task is unmasked"
        chosen[c.d] = best
        base.append(int(LA.base_pick(policy, c.seed_of)(c.mask, c.pos, c.task_xy, c.d)))
        nfree.append(int((c.mask == 0).sum()))
        return best

    w = LA.walk(a, t, inst_one, seed, action_of, mwt, max_time=max_time)
    assert w["ended"]
    o = oracle.OracleEnv(a, t, max_waiting_time=mwt, max_time=max_time).load(inst_one["depot"], inst_one["task_xy"], inst_one["req"], inst_one["dur"])
    r = o.rollout(0, 0, oracle.POLICY_INJECTED, cap_steps=max(w["n_steps"], 1), record=False, inj_leader=w["leader"],
                  inj_action=w["action"], inj_nfol=w["nfol"], inj_followers=w["followers"])
    assert r["n_steps"] == w["n_steps"]
    flags = DONE | (FINISHED if r["finished"].all() and r["returned"].all() else 0) | (TRUNCATED if r["truncated"] else 0)
    return dict(w, base_action=np.array(base, np.int32), n_unmasked=np.array(nfree, np.int32), result=r, o=o, flags=flags, a=a)


class Episode:
    """what O.assert_log reads of an episode: .o (the OracleEnv holding its route lists) and .a"""

    def __init__(self, w):
        self.o, self.a, self.w = w["o"], w["a"], w


# ---------------------------------------------------------------------------------- the shared cases
# name: (A, T, B, per-env sizes or None).  Tiny on purpose: a walker reference costs (decisions x unmasked actions) oracle walks.
TINY = {"5A8T": (5, 8, 4, None), "10A20T": (10, 20, 2, None)}
RAGGED = ("ragged", 10, 20, ((5, 8), (7, 12), (10, 20)))
INST_SEED, CHOICE_SEED = 83, 5


@functools.lru_cache(maxsize=None)
def instances(name):
    """(instances, choice seeds) of a tiny case: computed once, never changed"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    A, T, B, _ = TINY[name]
    return generate_batch(B, A, T, base_seed=INST_SEED + 3 * A + T), env_seeds(CHOICE_SEED, 0, B)


@functools.lru_cache(maxsize=None)
def walks(name, policy):
    """the lookahead walk of every env of a tiny case under a base policy: computed once, shared by every test, never changed"""
    A, T, B, _ = TINY[name]
    inst, seeds = instances(name)
    return [lookahead_walk(A, T, O.one(inst, b), int(seeds[b]), policy) for b in range(B)]


@functools.lru_cache(maxsize=None)
def ragged_instances():
    """a LOADED ragged batch: dims 10 / 20 with env sizes (5, 8), (7, 12), (10, 20); padded as load_instances takes it"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_instance
    _, A, T, sizes = RAGGED
    B = len(sizes)
    inst = dict(depot=np.zeros((B, 2)), task_xy=np.zeros((B, T, 2)), req=np.ones((B, T), np.int32), dur=np.zeros((B, T)),
                n_agents=np.array([s[0] for s in sizes], np.int32), n_tasks=np.array([s[1] for s in sizes], np.int32))
    for b, (a, t) in enumerate(sizes):
        one = generate_instance(a, t, INST_SEED + 500 + b)
        inst["depot"][b] = one["depot"]
        inst["task_xy"][b, :t], inst["req"][b, :t], inst["dur"][b, :t] = one["task_xy"], one["req"], one["dur"]
    return inst, env_seeds(CHOICE_SEED + 1, 0, B)


@functools.lru_cache(maxsize=None)
def ragged_walks(policy="nearest"):
    _, A, T, sizes = RAGGED
    inst, seeds = ragged_instances()
    return [lookahead_walk(a, t, O.one(inst, b, t), int(seeds[b]), policy) for b, (a, t) in enumerate(sizes)]


# ---------------------------------------------------------------------------------- windows: a few lookahead decisions deep in an episode
def most_abandoned(o):
    """the largest number of abandonments of one agent so far (the 17th of an agent goes to the overflow count table)"""
    n = np.zeros(o.A, np.int64)
    for t in range(o.T):
        n += np.bincount(o.abandoned(t), minlength=o.A)
    return int(n.max())


def replay(a, t, inst_one, w, mwt, max_time=LA.MAX_TIME):
    """The oracle's own rollout of a walk's choices: (the OracleEnv, holding the route lists; its result; the flags the env's header holds
    after the episode, as lookahead_walk states them)."""
    import oracle
    o = oracle.OracleEnv(a, t, max_waiting_time=mwt, max_time=max_time).load(inst_one["depot"], inst_one["task_xy"], inst_one["req"], inst_one["dur"])
    r = o.rollout(0, 0, oracle.POLICY_INJECTED, cap_steps=max(w["n_steps"], 1), record=False, inj_leader=w["leader"],
                  inj_action=w["action"], inj_nfol=w["nfol"], inj_followers=w["followers"])
    assert r["n_steps"] == w["n_steps"]
    flags = DONE | (FINISHED if r["finished"].all() and r["returned"].all() else 0) | (TRUNCATED if r["truncated"] else 0)
    return o, r, flags


def lookahead_window(a, t, inst_one, seed, policy, mwt, d0, k, max_time=LA.MAX_TIME):
    """LA.walk(..., stop=d0 + k): decisions < d0 take the base policy's pick, decisions d0 .. d0 + k - 1 the lookahead rule -- no
    unmasked task: the depot; exactly one: that task; otherwise every unmasked action is valued by the oracle's result of
    LA.policy_walk(..., forced={every earlier choice, d: act}), and the largest LA.pair wins, strict > in ascending order.
    Returns the walk's dict (o: the OracleEnv in front of decision d0 + k, or where the episode ended) plus chosen {d: action} for every
    decision < d0 + k and facts, per window decision dict(d, n_unmasked, most0: most_abandoned in front of it, most1: (min, max) of it at the end of
    the inner episodes, at_max_time / truncated: inner episodes that ended with now >= max_time / under the oracle's guard, tie: the
    best pair belongs to two actions, differs: the choice is not the base policy's, members: the longest member list of a task)."""
    seed = int(seed)
    chosen, facts = {}, []

    def action_of(c):
        base = int(LA.base_pick(policy, c.seed_of)(c.mask, c.pos, c.task_xy, c.d))
        if c.d < d0:
            chosen[c.d] = base                  # forced in the inner walks too: they take the prefix without asking the policy again
            return base
        free = np.flatnonzero(c.mask == 0)
        assert len(free) and (c.mask[0] == 0) == bool(c.mask[1:].all()), "the depot is allowed iff no task is"
        f = dict(d=c.d, n_unmasked=len(free), most0=most_abandoned(c.o), most1=None, at_max_time=0, truncated=0, tie=False,
                 members=max(len(c.o.members(j)) for j in range(t)))
        best = int(free[0])
        if len(free) > 1:
            pairs, most = [], []
            for act in free:
                w = LA.policy_walk(a, t, inst_one, seed, policy, mwt, forced={**chosen, c.d: int(act)}, max_time=max_time)
                r = LA.result(a, t, inst_one, w, mwt, max_time)
                pairs.append(LA.pair(r))
                most.append(most_abandoned(w["o"]))
                f["at_max_time"] += w["o"].now >= max_time
                f["truncated"] += bool(r["truncated"])
            best, best_pair = None, None
            for act, p in zip(free, pairs):
                if best is None or p > best_pair:
                    best, best_pair = int(act), p
            f.update(most1=(min(most), max(most)), tie=pairs.count(best_pair) > 1)
        f["differs"] = best != base
        chosen[c.d] = best
        facts.append(f)
        return best

    w = LA.walk(a, t, inst_one, seed, action_of, mwt, stop=d0 + k, max_time=max_time)
    return dict(w, chosen=chosen, facts=facts, a=a, t=t)


def window_tail(a, t, inst_one, seed, policy, mwt, chosen, max_time=LA.MAX_TIME):
    """The whole episode made of the prefix, the window (chosen: lookahead_window's) and the base policy to the end: the walk plus
    result, o (the OracleEnv of the oracle's replay, for its route lists), flags and a, as lookahead_walk returns them."""
    w = LA.policy_walk(a, t, inst_one, int(seed), policy, mwt, forced=dict(chosen), max_time=max_time)
    assert w["ended"]
    o, r, flags = replay(a, t, inst_one, w, mwt, max_time)
    return dict(w, result=r, o=o, flags=flags, a=a)


def stopped_state(w):
    """What the getters of a handle must hold where a window walk stopped (w: lookahead_window's, cut by its stop): member lists,
    abandonment counts, the task and agent side, now, and the route lists -- read once; the waiting sums need the one call the oracle
    makes at an episode's end (as removal_ref.assert_handover), which is made last."""
    import oracle
    o, a, t = w["o"], w["a"], w["t"]
    assert not w["ended"], "the episode ended inside the window"
    members = [o.members(j) for j in range(t)]
    abc = np.zeros((a, t), np.int16)
    for j in range(t):
        abc[:, j] = np.bincount(o.abandoned(j), minlength=a)
    routes = [o.route(i) for i in range(a)]
    now, fin = o.now, o.final()
    oracle.lib().orc_finish_episode(o._h)
    end = o.final()
    return dict(members=members, abc=abc, routes=routes, now=now, tasks={k: fin[k] for k in ("n_members", "n_abandoned", "feasible",
                "finished", "time_start", "time_finish")}, travel_dist=end["travel_dist"], returned=end["returned"],
                agent_wait=end["agent_wait"], task_wait=end["task_wait"], decisions=w["n_steps"])


class Stopped:
    """what O.assert_log reads, from a stopped_state"""

    def __init__(self, s, a):
        self.a, self.o = a, self
        self._routes = s["routes"]

    def route(self, i):
        return self._routes[i]


# id: A, T, B, mwt, base policy, kw: handle keywords, sizes: per-env sizes (a ragged batch), req: drawn from 1..that, and the window:
# at = the share of the base policy's own oracle episode that lies in front of it (one for the batch, or one per env), K decisions.
# d0 comes from the base policy's oracle episode alone, nothing a device returns.
RAGGED_WINDOW_SIZES = ((70, 130), (64, 64), (65, 128), (64, 129), (70, 65), (1, 130), (20, 66), (66, 127))    # test_gpu_relay.RAGGED_SIZES
WINDOWS = {
    "spill-clean": dict(A=10, T=20, B=2, mwt=1.0, policy="nearest", at=0.0, K=4),
    "spill-saved": dict(A=10, T=20, B=2, mwt=1.0, policy="nearest", at=0.5, K=4),
    "spill-mixed": dict(A=10, T=20, B=3, mwt=1.0, policy="first", at=0.1, K=4),
    "s20x50-spill": dict(A=20, T=50, B=2, mwt=2.0, policy="nearest", at=0.8, K=3),
    "lay64": dict(A=30, T=60, B=2, mwt=2.0, policy="nearest", at=0.7, K=3),
    "no-depot-lane": dict(A=10, T=64, B=2, mwt=2.0, policy="nearest", at=0.9, K=2),
    "mc": dict(A=50, T=200, B=2, mwt=1.5, policy="nearest", at=(0.87, 0.9), K=3),
    "c5": dict(A=100, T=500, B=2, mwt=2.0, policy="nearest", at=(0.95, 0.985), K=2),
    "g2x3": dict(A=70, T=130, B=2, mwt=1.0, policy="random", at=0.85, K=3),
    "g-ragged": dict(A=70, T=130, B=8, mwt=1.0, policy="nearest", at=0.8, K=2, sizes=RAGGED_WINDOW_SIZES),
    "rt": dict(A=70, T=260, B=2, mwt=2.0, policy="first", at=0.85, K=2),
    "wide": dict(A=24, T=9, B=2, mwt=2.0, policy="nearest", at=0.5, K=4, req=16, kw=dict(member_cap=16)),
}


@functools.lru_cache(maxsize=None)
def window_instances(name):
    """(instances in load_instances' keyword format, choice seeds, per-env (a, t)) of a window case: computed once, never changed"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    c = WINDOWS[name]
    A, T, B = c["A"], c["T"], c["B"]
    inst = generate_batch(B, A, T, base_seed=INST_SEED + 3 * A + T)
    if c.get("req"):
        inst["req"] = np.random.default_rng(INST_SEED).integers(1, c["req"] + 1, (B, T)).astype(np.int32)
    sz = [(A, T)] * B
    if c.get("sizes"):
        sz = [tuple(s) for s in c["sizes"]]
        inst["n_agents"], inst["n_tasks"] = np.array([s[0] for s in sz], np.int32), np.array([s[1] for s in sz], np.int32)
    return inst, env_seeds(CHOICE_SEED, 0, B), sz


@functools.lru_cache(maxsize=None)
def window_starts(name):
    """d0 per env: the case's share of the decisions of the base policy's own oracle episode"""
    c = WINDOWS[name]
    inst, seeds, sz = window_instances(name)
    n = [O.episodes(a, t, O.one(inst, b, t), seeds[b], c["policy"], 1, c["mwt"])[0]["n_steps"] for b, (a, t) in enumerate(sz)]
    at = c["at"] if isinstance(c["at"], tuple) else (c["at"],) * len(n)
    return tuple(int(f * x) for f, x in zip(at, n)), tuple(n)


@functools.lru_cache(maxsize=None)
def windows(name):
    """per env of a window case dict(d0, K, window: lookahead_window's walk, stop: its stopped_state, tail: window_tail's episode):
    computed once, shared by the CPU and the GPU test, never changed"""
    c = WINDOWS[name]
    inst, seeds, sz = window_instances(name)
    d0s, _ = window_starts(name)
    out = []
    for b, (a, t) in enumerate(sz):
        one = O.one(inst, b, t)
        w = lookahead_window(a, t, one, seeds[b], c["policy"], c["mwt"], d0s[b], c["K"])
        tail = window_tail(a, t, one, seeds[b], c["policy"], c["mwt"], w["chosen"])
        out.append(dict(d0=d0s[b], K=c["K"], window=w, stop=stopped_state(w), tail=tail))
    return out


def window_sim_kind(name):
    """the Sim<> instantiation a window case's handle launches (roofline.sim_kind_name: csrc/plan.hpp's sim_kind)"""
    from dcmrta_amd.roofline import sim_kind_name
    c = WINDOWS[name]
    return sim_kind_name(c["A"], c["T"], ragged=bool(c.get("sizes")), wide=c.get("kw", {}).get("member_cap", 5) > 5)


# the renewing form at an MG shape: a generated 50A/200T handle whose lookahead window lies across the end of its first episode
RENEWING = dict(A=50, T=200, B=2, mwt=1.5, policy="nearest", stride=100, inst_seed=700, back=2)


@functools.lru_cache(maxsize=None)
def renewing_windows():
    """(instance seeds, choice seeds, per env dict(d0: `back` decisions in front of the end of the base policy's oracle episode, end:
    the decisions of the episode that takes the lookahead rule from d0 on, K = end - d0 + 1: one decision falls behind the restart,
    window: that episode's lookahead_window, result: its oracle result))."""
    from dcmrta_amd.choice import env_seeds
    from renewal_ref import host_instance
    c = RENEWING
    A, T, B = c["A"], c["T"], c["B"]
    inst_seeds, seeds = np.arange(c["inst_seed"], c["inst_seed"] + B, dtype=np.uint64), env_seeds(CHOICE_SEED + 4, 0, B)
    out = []
    for b in range(B):
        one = host_instance(A, T, int(inst_seeds[b]), 5)[1]
        n = O.episodes(A, T, one, seeds[b], c["policy"], 1, c["mwt"])[0]["n_steps"]
        d0 = n - c["back"]
        w = lookahead_window(A, T, one, seeds[b], c["policy"], c["mwt"], d0, 1 << 30)
        assert w["ended"]
        out.append(dict(d0=d0, end=w["n_steps"], K=w["n_steps"] - d0 + 1, window=w, result=replay(A, T, one, w, c["mwt"])[1]))
    return inst_seeds, seeds, out
