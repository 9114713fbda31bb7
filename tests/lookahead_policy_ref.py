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


def lookahead_walk(a, t, inst_one, seed, policy, mwt=10.0):
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
            w = LA.policy_walk(a, t, inst_one, seed, policy, mwt, forced={**chosen, c.d: int(act)})
            p = LA.pair(LA.result(a, t, inst_one, w, mwt))
            if best is None or p > best_pair:
                best, best_pair = int(act), p
        assert best is not None, "the mask always allows an action: the depot when no task is unmasked"
        chosen[c.d] = best
        base.append(int(LA.base_pick(policy, c.seed_of)(c.mask, c.pos, c.task_xy, c.d)))
        nfree.append(int((c.mask == 0).sum()))
        return best

    w = LA.walk(a, t, inst_one, seed, action_of, mwt)
    assert w["ended"]
    o = oracle.OracleEnv(a, t, max_waiting_time=mwt).load(inst_one["depot"], inst_one["task_xy"], inst_one["req"], inst_one["dur"])
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
