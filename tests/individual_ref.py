"""Individual selection against the oracle (test infrastructure): Worker.run_test_IS (worker.py:159-198) on the oracle's step-wise
surface, as test_gpu_api.py::test_individual_selection_mode restates it -- per event next_decision, now, task_update, agent_update;
per decider in ascending id mask, agent_step(a, action), task_update, agent_update; then check_finished.  There is no
get_unique_group, no leader draw and no follower: a decision is one agent's agent_step.
The action of decision d is lookahead_ref.base_pick("random" if choice.explores(seed, d, q32) else policy, ...): "random" always takes
protocol slot 1.  The cases the CPU and the GPU tests share live here, each computed once."""
import functools

import numpy as np

import lookahead_ref as LA
import oracle_ref as O

DONE, FINISHED = 1, 2
Q25 = (1 << 32) // 4                       # floor(0.25 * 2^32)


def walk(a, t, inst_one, seed, policy, q32=0, mwt=10.0, max_time=100.0, d0=0, stop=None, action_of=None):
    """One oracle episode under individual selection from decision counter d0.  stop: walk only the first `stop` decisions (the walk
    then ends in front of the next one, possibly in the middle of an event).  action_of(mask, d) replaces the policy's pick (hand-over
    tests: the host's rule).
    Returns dict(decider, action, event: the ordinal of the decision's event, mask: in front of every decision taken, n_steps, ended, o: the OracleEnv where the walk left it, a,
    obs: (mask, task_status, agent_status) in front of the last decision taken, or None, and the facts the host tests assert:
    followers: decisions at which a later decider of the event stands where the decider stands and the picked task has vacancy > 1
    (leader-follower would draw followers); depot_beside: depot decisions with such a decider (leader-follower would send the group);
    at_max_time: the episode ended with now >= max_time)."""
    import oracle
    from dcmrta_amd.choice import explores
    seed = int(seed)
    o = oracle.OracleEnv(a, t, max_waiting_time=mwt, max_time=max_time).load(inst_one["depot"], inst_one["task_xy"], inst_one["req"], inst_one["dur"])
    task_xy = np.asarray(inst_one["task_xy"], np.float64)
    depot = (float(inst_one["depot"][0]), float(inst_one["depot"][1]))
    pos = [depot] * a
    deciders, actions, masks, events, obs, event = [], [], [], [], None, -1
    followers = depot_beside = 0
    finished, n, empty, cut = False, 0, 0, False
    while not finished and o.now < max_time and not cut:                    # worker.py:163
        ids, now = o.next_decision()                                        # :165
        o.now = now                                                         # :167
        o.task_update()                                                     # :168
        o.agent_update()                                                    # :169
        event += 1
        if not len(ids):
            empty += 1
            if empty > 4:                                                   # the zero-decider guard, as lookahead_ref.walk keeps it
                break
        else:
            empty = 0
        for i, ag in enumerate(int(x) for x in ids):                        # :170 ascending id
            if stop is not None and n >= stop:
                cut = True
                break
            d = d0 + n
            mask = o.mask()                                                 # :175-179
            tk = o.task_status(ag)
            if action_of is not None:
                action = int(action_of(mask, d))
            else:
                action = int(LA.base_pick("random" if explores(seed, d, q32) else policy, lambda _d: seed)(mask, pos[ag], task_xy, d))
            assert mask[action] == 0
            beside = any(pos[int(x)] == pos[ag] for x in ids[i + 1:])
            followers += beside and action >= 1 and int(tk[action, 0]) > 1
            depot_beside += beside and action == 0
            obs = (mask, tk, o.agent_status(ag))
            o.agent_step(ag, action)                                        # :185-186
            pos[ag] = (float(task_xy[action - 1, 0]), float(task_xy[action - 1, 1])) if action >= 1 else depot
            o.task_update()                                                 # :187
            o.agent_update()                                                # :188
            deciders.append(ag); actions.append(action); masks.append(mask); events.append(event)
            n += 1
        if not cut:
            finished = o.check_finished()                                   # :189
    return dict(decider=np.array(deciders, np.int32), action=np.array(actions, np.int32), event=np.array(events, np.int32), mask=np.array(masks, np.uint8).reshape(n, t + 1),
                n_steps=n, ended=not cut, o=o, a=a, obs=obs, followers=int(followers), depot_beside=int(depot_beside),
                at_max_time=(not cut) and o.now >= max_time)


def final(w):
    """The terminal results of a finished walk (orc_finish_episode + final()), computed once per walk, plus n_steps, flags (what the
    env's header holds: DONE, and FINISHED iff every agent returned and every task finished) and abandonments."""
    import oracle
    if "final" not in w:
        assert w["ended"], "only a whole episode has a result"
        oracle.lib().orc_finish_episode(w["o"]._h)
        r = w["o"].final()
        r["n_steps"] = w["n_steps"]
        r["flags"] = DONE | (FINISHED if r["finished"].all() and r["returned"].all() else 0)
        r["abandonments"] = int(r["n_abandoned"].sum())
        w["final"] = r
    return w["final"]


def episodes(a, t, inst_of, seed, policy, n, q32=0, mwt=10.0, max_time=100.0):
    """n consecutive episodes of one env, the decision counter running on; inst_of: the instance, or k -> the instance of episode k
    (where that returns (A_k, instance), episode k has that instance's own sizes)."""
    out, d0 = [], 0
    for k in range(n):
        i = inst_of(k) if callable(inst_of) else inst_of
        ak, tk = a, t
        if isinstance(i, tuple):
            ak, i = i
            tk = i["req"].shape[0]
        w = walk(ak, tk, i, seed, policy, q32, mwt, max_time, d0)
        final(w)
        out.append(w)
        d0 += w["n_steps"]
    return out


def abandoned_counts(w):
    """int16[a, t]: how often each agent was dropped from each task (dcm abandonment log's count table)"""
    o = w["o"]
    out = np.zeros((o.A, o.T), np.int16)
    for j in range(o.T):
        out[:, j] = np.bincount(o.abandoned(j), minlength=o.A)
    return out


# ---------------------------------------------------------------------------------- the shared cases
# id: A, T, B, max_waiting_time, max_time, handle keywords, req: requirements drawn from 1..that.  One per Sim<> instantiation of the
# general kernel (roofline.sim_kind_name); the multi-chunk shapes play to max_time 30 to keep the walks short.
CASES = {
    "6A12T": dict(A=6, T=12, B=4, mwt=10.0, max_time=100.0, sim="<20,50,true>"),
    "20A50T": dict(A=20, T=50, B=3, mwt=10.0, max_time=100.0, sim="<20,50,false>"),
    "30A60T": dict(A=30, T=60, B=2, mwt=10.0, max_time=100.0, sim="<64,64,true>"),
    "10A64T": dict(A=10, T=64, B=2, mwt=10.0, max_time=100.0, sim="<64,64,true>"),          # no depot lane: T + 1 > 64
    "50A200T": dict(A=50, T=200, B=2, mwt=10.0, max_time=30.0, sim="<50,200,false>"),
    "70A130T": dict(A=70, T=130, B=2, mwt=10.0, max_time=30.0, sim="<128,256,true>"),
    "70A260T": dict(A=70, T=260, B=2, mwt=10.0, max_time=30.0, sim="<0,0,false>"),
    "24A9T-wide": dict(A=24, T=9, B=2, mwt=10.0, max_time=100.0, req=16, kw=dict(member_cap=16), sim="<0,0,false,MW>"),
}
# max_waiting_time 2: abandonments, the log and its count table
SHORT_WAIT = {"6A12T-mwt2": dict(A=6, T=12, B=4, mwt=2.0, max_time=100.0), "20A50T-mwt2": dict(A=20, T=50, B=3, mwt=2.0, max_time=100.0)}
ALL = {**CASES, **SHORT_WAIT}
POLICIES = (("random", 0), ("first", 0), ("nearest", 0), ("nearest", Q25))
INST_SEED, CHOICE_SEED = 211, 17
RAGGED = dict(A=20, T=50, sizes=((6, 12), (20, 50), (13, 31), (1, 50)))
RENEWING = dict(A=10, T=20, B=3, stride=100, inst_seed=900)


def handle_kw(name):
    c = ALL[name]
    return dict(individual_selection=True, max_waiting_time=c["mwt"], max_time=c["max_time"], **c.get("kw", {}))


@functools.lru_cache(maxsize=None)
def instances(name):
    """(instances, choice seeds) of a case: computed once, never changed"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    c = ALL[name]
    A, T, B = c["A"], c["T"], c["B"]
    inst = generate_batch(B, A, T, base_seed=INST_SEED + 3 * A + T)
    if c.get("req"):
        inst["req"] = np.random.default_rng(INST_SEED).integers(1, c["req"] + 1, (B, T)).astype(np.int32)
    return inst, env_seeds(CHOICE_SEED, 0, B)


@functools.lru_cache(maxsize=None)
def walks(name, policy, q32=0, n=1):
    """[b][k]: episode k of env b of a case under (policy, explore_q32), individual selection: computed once, shared, never changed"""
    c = ALL[name]
    inst, seeds = instances(name)
    return [episodes(c["A"], c["T"], O.one(inst, b), int(seeds[b]), policy, n, q32, c["mwt"], c["max_time"]) for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def grouped(name, policy):
    """the leader-follower episode of every env of a case (lookahead_ref.policy_walk and the oracle's replay of it)"""
    c = ALL[name]
    inst, seeds = instances(name)
    out = []
    for b in range(c["B"]):
        w = LA.policy_walk(c["A"], c["T"], O.one(inst, b), int(seeds[b]), policy, c["mwt"], max_time=c["max_time"])
        out.append((w, LA.result(c["A"], c["T"], O.one(inst, b), w, c["mwt"], c["max_time"])))
    return out


@functools.lru_cache(maxsize=None)
def ragged_instances():
    """a LOADED ragged batch, padded as load_instances takes it, and its choice seeds"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_instance
    A, T, sizes = RAGGED["A"], RAGGED["T"], RAGGED["sizes"]
    B = len(sizes)
    inst = dict(depot=np.zeros((B, 2)), task_xy=np.zeros((B, T, 2)), req=np.ones((B, T), np.int32), dur=np.zeros((B, T)),
                n_agents=np.array([s[0] for s in sizes], np.int32), n_tasks=np.array([s[1] for s in sizes], np.int32))
    for b, (a, t) in enumerate(sizes):
        one = generate_instance(a, t, INST_SEED + 500 + b)
        inst["depot"][b] = one["depot"]
        inst["task_xy"][b, :t], inst["req"][b, :t], inst["dur"][b, :t] = one["task_xy"], one["req"], one["dur"]
    return inst, env_seeds(CHOICE_SEED + 1, 0, B)


@functools.lru_cache(maxsize=None)
def ragged_walks(policy, q32=0, n=2):
    inst, seeds = ragged_instances()
    return [episodes(a, t, O.one(inst, b, t), int(seeds[b]), policy, n, q32) for b, (a, t) in enumerate(RAGGED["sizes"])]


@functools.lru_cache(maxsize=None)
def renewing_walks(policy, q32=0):
    """(instance seeds, choice seeds, [b][k]) of a generated uniform batch that renews its instances with RENEWING's stride: episode k
    plays instance seed + k * stride (renewal_ref.host_instance)"""
    from dcmrta_amd.choice import env_seeds
    from renewal_ref import host_instance
    c = RENEWING
    A, T, B = c["A"], c["T"], c["B"]
    inst_seeds, seeds = np.arange(c["inst_seed"], c["inst_seed"] + B, dtype=np.uint64), env_seeds(CHOICE_SEED + 3, 0, B)
    out = [episodes(A, T, lambda k, b=b: host_instance(A, T, int(inst_seeds[b]) + k * c["stride"], 5)[1], int(seeds[b]), policy, 2, q32)
           for b in range(B)]
    return inst_seeds, seeds, out


class Episode:
    """what O.assert_log reads of a walk: .o (the OracleEnv holding its route lists) and .a"""

    def __init__(self, w):
        self.o, self.a, self.w = w["o"], w["a"], w


def mid_event_stop(w, after):
    """the first k > after at which decisions k - 1 and k of a walk belong to one event: a launch of k decisions stops inside it"""
    ev = w["event"]
    for k in range(after + 1, len(ev)):
        if ev[k - 1] == ev[k]:
            return k
    raise AssertionError("no event with two deciders behind decision %d" % after)
