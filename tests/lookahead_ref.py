"""Lookahead against the oracle (test infrastructure): one oracle episode walked through the step-wise API with the action of every
decision given by a function and the seed of the draws allowed to switch at a decision -- what a forked env plays --, the `nearest`
pick restated in Python, and the values a one-step lookahead over a base policy must return.  The walk yields the choices; the
episode's result is the oracle's own rollout with those choices injected."""
import functools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import oracle_ref as O

MAX_TIME = 100.0


@functools.lru_cache(maxsize=1 << 16)
def distance(ax, ay, bx, by):
    """calculate_eulidean_distance (env/task_env.py:161-163) as the kernels and the oracle compute it: sqrt(fma(dy, dy, dx * dx)) in
    fp64.  dx * dx is rounded, the fma is exact before its one rounding (Fraction holds the sum exactly; float() of a Fraction rounds
    correctly), and math.sqrt is correctly rounded."""
    dx, dy = float(ax) - float(bx), float(ay) - float(by)
    return math.sqrt(float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx)))


def pick_first(mask, pos, task_xy):
    """the lowest unmasked action (the depot, 0, when nothing is unmasked)"""
    free = np.flatnonzero(mask == 0)
    return int(free[0]) if len(free) else 0


def pick_nearest(mask, pos, task_xy):
    """policy_pick's `nearest`: the depot if it is unmasked, else the unmasked task with the smallest distance from the deciding agent,
    strict < in ascending task order, so a tie goes to the lowest index (the depot when nothing is unmasked)."""
    if not mask[0]:
        return 0
    best, bd = 0, 0.0
    for k in range(1, len(mask)):
        if not mask[k]:
            dd = distance(pos[0], pos[1], task_xy[k - 1, 0], task_xy[k - 1, 1])
            if best == 0 or dd < bd:
                best, bd = k, dd
    return best


def pick_random(seed_of):
    """the random policy's action: slot 1 of decision d over the unmasked actions, under the seed the walk draws decision d from"""
    from dcmrta_amd.choice import below, draw

    def pick(mask, pos, task_xy, d):
        free = np.flatnonzero(mask == 0)
        return int(free[below(draw(seed_of(d), d, 1), len(free))])
    return pick


def base_pick(policy, seed_of):
    if policy == "random":
        return pick_random(seed_of)
    f = {"first": pick_first, "nearest": pick_nearest}[policy]
    return lambda mask, pos, task_xy, d: f(mask, pos, task_xy)


def walk(a, t, inst_one, seed, action_of, mwt=10.0, switch=None, stop=None, max_time=MAX_TIME, after_task_update=None):
    """One oracle episode through the step-wise API (the loop of worker.py:45-87, as removal_ref.walk_episode restates it) with
    every decision's action given by action_of(c) -> action; c.d: the decision counter, c.mask, c.leader, c.pos: the deciding agent's
    fp64 location, c.task_xy, c.seed_of: d -> the seed decision d draws from, c.o: the OracleEnv in front of the decision.
    switch = (d_s, seed_2): decisions d >= d_s draw leader, action and followers from seed_2 -- a copy of the env made in front of
    decision d_s and given that seed.  stop: walk only the first `stop` decisions.  after_task_update(o): called behind every task_update
    pass of the walk.
    Returns dict(leader, action, nfol, followers[n, a], mask: the mask in front of every decision taken, n_steps, ended,
    seed_of) -- the choices in the form OracleEnv.rollout injects -- and o, the OracleEnv where the walk left it (a walk that `stop`
    cut: in front of decision `stop`)."""
    import oracle
    from dcmrta_amd.choice import below, draw
    seed_of = (lambda d: seed) if switch is None else (lambda d: switch[1] if d >= switch[0] else seed)
    o = oracle.OracleEnv(a, t, max_waiting_time=mwt, max_time=max_time).load(inst_one["depot"], inst_one["task_xy"], inst_one["req"], inst_one["dur"])
    task_xy = np.asarray(inst_one["task_xy"], np.float64)
    pos = [(float(inst_one["depot"][0]), float(inst_one["depot"][1]))] * a
    pos = list(pos)
    leaders, actions, nfols, fols, masks = [], [], [], [], []
    finished, d, empty, cut = False, 0, 0, False
    while not finished and o.now < max_time and not cut:                    # worker.py:45
        ids, now = o.next_decision()                                        # :47
        groups = o.get_unique_group(ids) if len(ids) else []               # :48
        o.now = now                                                         # :49
        o.task_update()                                                     # :50
        if after_task_update:
            after_task_update(o)
        o.agent_update()                                                    # :51
        if not groups:
            empty += 1
            if empty > 4:
                break
        else:
            empty = 0
        for group in groups:                                                # :52
            while group and not cut:                                        # :53
                if stop is not None and d >= stop:
                    cut = True
                    break
                leader = group[below(draw(seed_of(d), d, 0), len(group))]   # :54
                mask, tk = o.mask(), o.task_status(leader)
                action = int(action_of(SimpleNamespace(d=d, mask=mask, leader=leader, pos=pos[leader], task_xy=task_xy, seed_of=seed_of, o=o)))
                vacancy = int(tk[action, 0]) if action >= 1 else len(group)  # :327 (the status may be stale)
                group.remove(leader)                                        # :328
                step = [leader]
                if vacancy > 1:                                             # :330-333
                    for j in range(min(vacancy - 1, len(group))):
                        step.append(group.pop(below(draw(seed_of(d), d, 2 + j), len(group))))
                for m in step:
                    o.agent_step(m, action)                                 # :338-340
                    pos[m] = (float(task_xy[action - 1, 0]), float(task_xy[action - 1, 1])) if action >= 1 else \
                        (float(inst_one["depot"][0]), float(inst_one["depot"][1]))
                o.task_update()                                             # :74
                if after_task_update:
                    after_task_update(o)
                o.agent_update()                                            # :76
                leaders.append(leader); actions.append(action); nfols.append(len(step) - 1); masks.append(mask)
                fols.append(step[1:] + [-1] * (a - len(step) + 1))
                d += 1
            if cut:
                break
        if not cut:
            finished = o.check_finished()                                   # :85
    n = len(actions)
    return dict(leader=np.array(leaders, np.int32), action=np.array(actions, np.int32), nfol=np.array(nfols, np.int32),
                followers=np.array(fols, np.int16).reshape(n, a), mask=np.array(masks, np.uint8).reshape(n, t + 1),
                n_steps=n, ended=not cut, seed_of=seed_of, o=o)


def result(a, t, inst_one, w, mwt=10.0, max_time=MAX_TIME):
    """The oracle's own rollout of a finished walk's choices, every one of them injected: the episode's terminal results
    (OracleEnv.rollout's dict; n_steps must come out as the walk's)."""
    import oracle
    assert w["ended"], "only a whole episode has a result"
    o = oracle.OracleEnv(a, t, max_waiting_time=mwt, max_time=max_time).load(inst_one["depot"], inst_one["task_xy"], inst_one["req"], inst_one["dur"])
    r = o.rollout(0, 0, oracle.POLICY_INJECTED, cap_steps=max(w["n_steps"], 1), record=False, inj_leader=w["leader"],
                  inj_action=w["action"], inj_nfol=w["nfol"], inj_followers=w["followers"])
    assert r["n_steps"] == w["n_steps"], ("the injected rollout took another number of decisions", r["n_steps"], w["n_steps"])
    return r


def policy_walk(a, t, inst_one, seed, policy, mwt=10.0, switch=None, forced=None, stop=None, max_time=MAX_TIME):
    """walk() under a base policy ("first", "nearest", "random"); forced = {d: action}: those decisions take that action instead."""
    forced = forced or {}

    def action_of(c):
        return forced[c.d] if c.d in forced else base_pick(policy, c.seed_of)(c.mask, c.pos, c.task_xy, c.d)
    return walk(a, t, inst_one, seed, action_of, mwt, switch, stop, max_time)


def lookahead_values(a, t, inst_one, seed, d, policy="nearest", mwt=10.0, max_time=MAX_TIME):
    """What Lookahead.values() returns for an env in front of decision d of its `policy` episode (the decisions before d taken by the
    policy): reward f64[t + 1], finished i32[t + 1], NaN / -1 where the mask in front of decision d forbids the action; and the mask.
    None when the episode has fewer than d + 1 decisions."""
    head = policy_walk(a, t, inst_one, seed, policy, mwt, stop=d + 1, max_time=max_time)
    if head["n_steps"] <= d:
        return None
    mask = head["mask"][d]
    reward, finished = np.full(t + 1, np.nan), np.full(t + 1, -1, np.int32)
    for act in np.flatnonzero(mask == 0):
        r = result(a, t, inst_one, policy_walk(a, t, inst_one, seed, policy, mwt, forced={d: int(act)}, max_time=max_time), mwt, max_time)
        reward[act], finished[act] = r["reward"], int(r["finished"].sum())
    return reward, finished, mask


def routes_walk(a, t, inst_one, seed, route_task, mwt=10.0, max_time=MAX_TIME):
    """walk() with every decision's action read from logged routes (route_task[a, cap], -1 = depot: the layout of enable_route_log):
    the leader's next entry -- every agent_step appends one to the route of the agent that takes it, in the oracle as in the log"""
    return walk(a, t, inst_one, seed, lambda c: int(route_task[c.leader, len(c.o.route(c.leader)[0])]) + 1, mwt, max_time=max_time)


def pair(r):
    """(finished tasks, reward) of an oracle result: the order of the best log and of Lookahead.plan()"""
    return int(r["finished"].sum()), float(r["reward"])


summary_row = O.summary_row
