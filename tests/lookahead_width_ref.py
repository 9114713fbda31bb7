"""The width-limited device lookahead (dcm_rollout_lookahead_width; BatchedTaskEnv.rollout(policy, lookahead=True, width=W)) against
the oracle (test infrastructure): the rule of include/dcmrta_env.h restated on the step-wise oracle walker of lookahead_ref.py -- the
candidate list by repeated `nearest` picks, the index tie-break of the best pair, and the count of the inner episodes' decisions.  The
cases the CPU and the GPU tests share live here, each computed once."""
import functools

import numpy as np

import lookahead_policy_ref as LP
import lookahead_ref as LA
import oracle_ref as O


def candidates(mask, pos, task_xy, width):
    """The actions `nearest` would pick one after the other if each pick were masked for the next: at most `width` of them, in that
    order -- ascending (rounded fp64 distance from pos, index)."""
    m, out = np.array(mask, copy=True), []
    for _ in range(width):
        act = LA.pick_nearest(m, pos, task_xy)
        if act == 0:
            break
        out.append(act)
        m[act] = 1
    return out


def decide(a, t, inst_one, seed, policy, mwt, width, chosen, c, max_time=LA.MAX_TIME):
    """Decision c.d under `lookahead, width`: (action, inner decisions, facts).  chosen: every earlier decision's action, forced in the
    inner walks.  An inner episode costs the decisions of its LA.policy_walk behind decision c.d: n_steps - d - 1.
    facts: n_unmasked, cand (the valued actions in the order they were valued; empty where nothing was), dist ({action: distance} of
    every unmasked task), pairs ({action: LA.pair} of the valued ones)."""
    tasks = [int(k) for k in np.flatnonzero(c.mask[1:] == 0) + 1]
    dist = {k: LA.distance(c.pos[0], c.pos[1], c.task_xy[k - 1, 0], c.task_xy[k - 1, 1]) for k in tasks}
    f = dict(d=c.d, n_unmasked=len(tasks), cand=[], dist=dist, pairs={})
    if len(tasks) == 0:
        return 0, 0, f
    if len(tasks) == 1:
        return tasks[0], 0, f
    if width == 1:
        return LA.pick_nearest(c.mask, c.pos, c.task_xy), 0, f
    cand = tasks if (width == 0 or width >= len(tasks)) else candidates(c.mask, c.pos, c.task_xy, width)
    best, best_pair, inner = None, None, 0
    for act in cand:
        w = LA.policy_walk(a, t, inst_one, seed, policy, mwt, forced={**chosen, c.d: act}, max_time=max_time)
        p = LA.pair(LA.result(a, t, inst_one, w, mwt, max_time))
        inner += w["n_steps"] - c.d - 1
        f["pairs"][act] = p
        if best is None or p > best_pair or (p == best_pair and act < best):
            best, best_pair = act, p
    f["cand"] = list(cand)
    return best, inner, f


def width_window(a, t, inst_one, seed, policy, mwt, width, d0=0, k=None, max_time=LA.MAX_TIME):
    """LA.walk under the width-limited rule, built like LP.lookahead_window: decisions < d0 take the base policy's pick, decisions d0 ..
    d0 + k - 1 (k None: to the episode's end) the rule of decide().  Returns the walk's dict plus chosen {d: action}, facts (decide's,
    per window decision), inner (the inner decisions of the whole window), a and t."""
    seed = int(seed)
    chosen, facts, inner = {}, [], [0]

    def action_of(c):
        if c.d < d0:
            chosen[c.d] = int(LA.base_pick(policy, c.seed_of)(c.mask, c.pos, c.task_xy, c.d))
            return chosen[c.d]
        act, n, f = decide(a, t, inst_one, seed, policy, mwt, width, chosen, c, max_time)
        chosen[c.d] = act
        inner[0] += n
        facts.append(f)
        return act

    w = LA.walk(a, t, inst_one, seed, action_of, mwt, stop=None if k is None else d0 + k, max_time=max_time)
    return dict(w, chosen=chosen, facts=facts, inner=inner[0], a=a, t=t)


def width_walk(a, t, inst_one, seed, policy, width, mwt=10.0, max_time=LA.MAX_TIME):
    """A whole episode under the width-limited rule: LP.lookahead_walk's dict (result, o: the OracleEnv of the oracle's replay, flags,
    a) plus inner and facts."""
    w = width_window(a, t, inst_one, seed, policy, mwt, width, max_time=max_time)
    assert w["ended"]
    o, r, flags = LP.replay(a, t, inst_one, w, mwt, max_time)
    return dict(w, result=r, o=o, flags=flags)


# ---------------------------------------------------------------------------------- the shared cases
@functools.lru_cache(maxsize=None)
def walks(name, policy, width):
    """the width-limited walk of every env of a tiny case of LP.TINY: computed once, shared by every test, never changed"""
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    return [width_walk(A, T, O.one(inst, b), int(seeds[b]), policy, width) for b in range(B)]


@functools.lru_cache(maxsize=None)
def nearest_walks(name):
    """the `nearest` episode of every env of a tiny case, on the same walker"""
    A, T, B, _ = LP.TINY[name]
    inst, seeds = LP.instances(name)
    return [LA.policy_walk(A, T, O.one(inst, b), int(seeds[b]), "nearest") for b in range(B)]


@functools.lru_cache(maxsize=None)
def ragged_walks(policy="nearest", width=2):
    _, A, T, sizes = LP.RAGGED
    inst, seeds = LP.ragged_instances()
    return [width_walk(a, t, O.one(inst, b, t), int(seeds[b]), policy, width) for b, (a, t) in enumerate(sizes)]


# Windows of K width-limited decisions.  id: A, T, B, mwt, base policy, width, at: the share of the base policy's own oracle episode in
# front of the window (d0 comes from the oracle alone), K, and how the generated instances are changed:
#   twins: task j + T/2 lies where task j lies, so equal distances are certain by construction, not by arithmetic
#   same = (i, j): tasks i and j lie at one point, nearer to the depot than every other task
# ties-*: B = 2, two decisions from d0 = 0.  Width 3 cuts a pair of twins in two; width 4 takes both.
# The shape cases: one per form of Sim::next_nearest_task -- one chunk (lane = task), CT != 0 unrolled with and without the XY
# registers, the runtime loop.
WINDOWS = {
    "ties-cut": dict(A=5, T=8, B=2, mwt=10.0, policy="nearest", width=3, at=0.0, K=2, twins=True),
    "ties-in": dict(A=5, T=8, B=2, mwt=10.0, policy="first", width=4, at=0.0, K=2, twins=True),
    "one-chunk-64": dict(A=10, T=64, B=2, mwt=2.0, policy="nearest", width=3, at=0.5, K=2),
    "lane-owns-two": dict(A=10, T=70, B=2, mwt=2.0, policy="nearest", width=3, at=0.0, K=2, same=(3, 67)),
    "xy-registers": dict(A=50, T=200, B=2, mwt=1.5, policy="nearest", width=3, at=0.5, K=1),
    "runtime-loop": dict(A=8, T=260, B=2, mwt=2.0, policy="first", width=3, at=0.3, K=2),
}
SIM_KINDS = {"ties-cut": "<20,50,true>", "ties-in": "<20,50,true>", "one-chunk-64": "<64,64,true>", "lane-owns-two": "<128,256,true>",
             "xy-registers": "<50,200,false>", "runtime-loop": "<0,0,false>"}


@functools.lru_cache(maxsize=None)
def window_instances(name):
    """(instances in load_instances' keyword format, choice seeds) of a window case: computed once, never changed"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    c = WINDOWS[name]
    A, T, B = c["A"], c["T"], c["B"]
    inst = generate_batch(B, A, T, base_seed=LP.INST_SEED + 5 * A + T)
    inst = {k: np.array(v, copy=True) for k, v in inst.items()}
    if c.get("twins"):
        inst["task_xy"][:, T // 2:] = inst["task_xy"][:, :T // 2]
    if c.get("same"):
        i, j = c["same"]
        for b in range(B):
            d = [LA.distance(inst["depot"][b, 0], inst["depot"][b, 1], x, y) for x, y in inst["task_xy"][b]]
            inst["task_xy"][b, i] = inst["task_xy"][b, j] = (inst["depot"][b] + inst["task_xy"][b, int(np.argmin(d))]) / 2   # half way there
    return inst, env_seeds(LP.CHOICE_SEED + 6, 0, B)


@functools.lru_cache(maxsize=None)
def windows(name):
    """per env of a window case dict(d0, K, window: width_window's walk, stop: LP.stopped_state of it, tail: LP.window_tail's episode):
    computed once, shared by the CPU and the GPU test, never changed"""
    c = WINDOWS[name]
    inst, seeds = window_instances(name)
    A, T = c["A"], c["T"]
    out = []
    for b in range(c["B"]):
        one = O.one(inst, b)
        d0 = int(c["at"] * O.episodes(A, T, one, seeds[b], c["policy"], 1, c["mwt"])[0]["n_steps"]) if c["at"] else 0
        w = width_window(A, T, one, seeds[b], c["policy"], c["mwt"], c["width"], d0, c["K"])
        tail = LP.window_tail(A, T, one, seeds[b], c["policy"], c["mwt"], w["chosen"])
        out.append(dict(d0=d0, K=c["K"], window=w, stop=LP.stopped_state(w), tail=tail))
    return out


def cut_ties(f, width):
    """the W-th and the (W+1)-th nearest unmasked task of a decision lie at one distance"""
    order = sorted(f["dist"], key=lambda k: (f["dist"][k], k))
    return len(order) > width and f["dist"][order[width - 1]] == f["dist"][order[width]]


def candidate_ties(f):
    """two candidates of a decision lie at one distance"""
    d = [f["dist"][k] for k in f["cand"]]
    return len(set(d)) < len(d)


def value_ties(f):
    """the best pair of a decision belongs to two candidates"""
    p = list(f["pairs"].values())
    return bool(p) and p.count(max(p)) > 1
