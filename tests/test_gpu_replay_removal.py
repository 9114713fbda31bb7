"""Member removal in the two route-replay kernels above the golden shapes: k_replay_fast<2,2,...> (csrc/replay_fast.hpp: the wave-uniform
removal loop of its task_update, the byte-packed id word, the agents' own-lane abandonment log) with two agent chunks and two task
chunks at once, and k_replay (csrc/dcmrta_replay.hip: task_update_one / task_update_joined, the abandonment log and counts in the
handle's HBM scratch) with tasks beyond 128, under both scratch placements and with sixteen member slots -- against the oracle, exactly.

The routes are built here (routes_for): most routed tasks get exactly the agents they require, about a third one too few, some one
too many, and some routed tasks last 105 time units, so that the agent that worked one reaches its next task more than
max_waiting_time = 100 (env/task_env.py:564) after the others.  Two situations are planted per env (_plant): a task that abandons an
early visitor and is finished later by a pair, and a full list whose arrivals spread further than 100 (:262), which in a replay needs
a joiner that decides before the earliest member's own +100 event and arrives after it.

CPU part (no kernel involved): test_inputs_reach_every_removal_path shows from the oracle alone that the inputs hold what the kernels
can get wrong, and that no env raises, truncates, collects more than five members or abandons an agent more than twice.  That last
bound is structural: whichever rule removes it, an agent stays at a task that does not start until its own arrival + 100, and the
replay ends at 200 (:565), so every abandonment costs an agent 100 of the 200 time units; the abandonment log's overflow branch
(AB_CAP = 16 entries per agent) therefore cannot be reached in a replay, and there is no overflow case here, unlike the rollout tests.
Static cases are walked with the oracle's step-wise API (walk_static: oracle/dcmrta_oracle.c:633-670 without its reactive lines,
checked against execute_by_route), which shows the member lists around every task_update call.

GPU part: every (member_cap, placement) of a case with the replay log on against the oracle bit for bit, the same without the log
(LOG = false against LOG = true), removal-heavy / plain / removal-heavy routes on one handle, and the three placements against each
other."""
import time

import numpy as np
import pytest

RNG_SEED = 7
MWT, CUTOFF = 100.0, 200.0          # env/task_env.py:564-565, the constants of dcm_execute_routes
KEYS_EXACT = ("finished", "time_start", "time_finish", "task_wait", "n_members", "travel_dist", "returned", "agent_wait")
LOG_KEYS = ("route_len", "members", "feasible")
BAD_FLAGS = 4 | 8 | 16 | 64 | 128   # TRUNCATED, BAD_ACTION, OVERFLOW, TYPE_ERROR, WAIT_ORDER (dcmrta_amd/_lib.py)

# vis: None = static replay, () = reactive at the reference's constants (20, 20, 10, 100), a tuple = set_visibility(*vis).
# runs: (member_cap, placement) pairs.  inputs: the case whose instances and routes this one replays (default: its own).
CASES = {
    "f70x66": dict(A=70, T=66, B=4, vis=None, kernel="k_replay_fast", runs=((5, "auto"), (8, "auto"))),
    "f128x128": dict(A=128, T=128, B=4, vis=None, kernel="k_replay_fast", runs=((5, "auto"), (8, "auto"))),
    "f70x100r": dict(A=70, T=100, B=4, vis=(), kernel="k_replay_fast", runs=((5, "auto"),)),
    "f128x128r": dict(A=128, T=128, B=4, vis=(32, 32, 10, 128), kernel="k_replay_fast", runs=((8, "auto"),)),
    "f20x50": dict(A=20, T=50, B=4, vis=None, kernel="k_replay_fast", runs=((5, "auto"),)),
    "g20x130": dict(A=20, T=130, B=4, vis=None, kernel="k_replay", runs=((5, "lds"), (5, "hbm"), (16, "auto"))),
    "g100x500": dict(A=100, T=500, B=3, vis=None, kernel="k_replay", runs=((5, "lds"), (5, "hbm"), (8, "hbm"), (16, "auto"))),
    "g100x500r": dict(A=100, T=500, B=3, vis=(100, 100, 10, 500), kernel="k_replay", runs=((5, "lds"), (5, "hbm"))),
    "g70x66": dict(A=70, T=66, B=4, vis=None, kernel="k_replay", runs=((8, "lds"), (8, "hbm")), inputs="f70x66"),
}
RUNS = [(n, cap, pl) for n, c in CASES.items() for cap, pl in c["runs"]]
STATE_RUNS = [("f128x128", 8, "auto"), ("g100x500", 5, "hbm"), ("g100x500", 5, "lds")]
PLACEMENT_CASES = ["g100x500", "g100x500r"]

_inputs, _refs, _plain = {}, {}, {}


def _reactive(c):
    return c["vis"] is not None


def _schedule(c):
    return c["vis"] or (20, 20, 10, 100)


def test_cases_run_the_kernels_they_name():
    """roofline.replay_kernel_name (pinned to plan::replay_kind of csrc/plan.hpp by test_host.py) for the default placement; an
    explicit placement asks for the general kernel (plan.hpp).  The plan's two further conditions -- a route capacity below 32768 and
    the register-resident kernel's LDS need within 64 KiB -- hold by a wide margin: FL of csrc/replay_fast.hpp restated."""
    from dcmrta_amd.roofline import replay_kernel_name
    for name, c in CASES.items():
        A, T = c["A"], c["T"]
        _, routes = inputs(name)
        cap = max(len(r) for env in routes for r in env)
        for mc, placement in c["runs"]:
            auto = replay_kernel_name(A, T, mc, _reactive(c), _schedule(c)[3])
            assert (auto if placement == "auto" else "k_replay") == c["kernel"], (name, mc, placement)
            if c["kernel"] == "k_replay_fast":
                head = 4 * A * cap + 15 & ~15
                assert cap < 32768 and max(head + 24 * 128, 8 * T + 8 * A + 15 & ~15) + 12 * 128 + 16 * 128 <= 64 * 1024, name
    assert CASES["g70x66"]["inputs"] == "f70x66" and (CASES["g70x66"]["A"], CASES["g70x66"]["T"]) == (CASES["f70x66"]["A"], CASES["f70x66"]["T"])
    assert all(n in CASES and (cap, pl) in CASES[n]["runs"] for n, cap, pl in STATE_RUNS)


# ------------------------------------------------------------------------------------------------------------------- inputs
def _travel(p, q):
    return float(np.hypot(*(np.asarray(p) - np.asarray(q)))) / 0.2           # env/task_env.py:315, velocity :99


def _plant(depot, xy, req, dur, free_tasks, free_agents, routes):
    """Two planted situations, on the highest free tasks and agents (second lane chunks where the shape has them).

    finished after an abandonment: a requirement-2 task K, an early visitor E that goes straight to it, and a pair that first works
    a requirement-2 task S whose duration ends one time unit after E's +100 event: E leaves by the waiting rule, the pair completes K.

    spread rule (:262): a requirement-2 task K, X goes straight to it and arrives at x; Y first works a requirement-1 task S whose
    duration is set so that Y decides at x + 100 - d / 2 and arrives at x + 100 + d / 2, d = the travel time from S to K.  Y's join
    fills the list with a spread of 100 + d / 2, and the call removes X before its own +100 event."""
    by_req = lambda r: [t for t in sorted(free_tasks, reverse=True) if req[t] == r]
    two, one = by_req(2), by_req(1)
    agents = sorted(free_agents, reverse=True)
    if len(two) < 3 or len(one) < 1 or len(agents) < 5:
        return
    k1, s1, k2, s2 = two[0], two[2], two[1], one[0]
    e, p1, p2, x, y = agents[2], agents[0], agents[4], agents[1], agents[3]      # (the two plants' agents interleaved)
    dur[s1] = _travel(depot, xy[k1]) + MWT - _travel(depot, xy[s1]) + 1.0
    dur[k1] = 2.0
    routes[e] += [k1]; routes[p1] += [s1, k1]; routes[p2] += [s1, k1]
    d = _travel(xy[s2], xy[k2])
    dur[s2] = _travel(depot, xy[k2]) + MWT - _travel(depot, xy[s2]) - d / 2
    routes[x] += [k2]; routes[y] += [s2, k2]
    for t in (k1, s1, k2, s2):
        free_tasks.discard(t)
    for a in (e, p1, p2, x, y):
        free_agents.discard(a)


def routes_for(rng, A, depot, xy, req, dur, limit):
    """Routes of one env (lists of actions: task + 1, the depot action 0 last) over tasks < limit; dur is edited in place."""
    routes = [[] for _ in range(A)]
    free_tasks, free_agents = set(range(limit)), set(range(A))
    fixed = {0, 1, limit - 2, limit - 1}
    for m in range(64, limit, 64):
        fixed |= {m - 1, m, m + 1}
    fixed = {t for t in fixed if 0 <= t < limit}
    free_tasks -= fixed
    _plant(depot, xy, req, dur, free_tasks, free_agents, routes)
    planted = set(range(limit)) - free_tasks - fixed
    rest = sorted(free_tasks)
    extra = rng.choice(rest, size=min(len(rest), A // 3), replace=False).tolist() if rest else []
    routed = sorted(fixed | set(extra))
    for t in routed:
        if rng.random() < 0.15:
            dur[t] = 105.0
    for t in routed:
        u, r = rng.random(), int(req[t])
        n = max(r - 1, 1) if (u < 0.35 or t == limit - 1) else (r + 1 if (u < 0.5 and r <= 4) else r)
        pool = [a for a in sorted(free_agents) if len(routes[a]) < 3]
        for a in rng.choice(pool, size=min(n, len(pool)), replace=False).tolist() if pool else []:
            routes[a].append(t)
    out = []
    for a in range(A):
        r = list(routes[a])
        if not (set(r) & planted):
            rng.shuffle(r)
        out.append([t + 1 for t in r] + [0])
    return out


def inputs(name):
    """(instances, routes[B][A]) of a case: generated once, read-only afterwards"""
    name = CASES[name].get("inputs", name)
    if name not in _inputs:
        from dcmrta_amd.instances import generate_batch
        c = CASES[name]
        A, T, B = c["A"], c["T"], c["B"]
        rng = np.random.default_rng(RNG_SEED)
        inst = generate_batch(B, A, T, base_seed=4000 + T)
        inst["dur"] = rng.random((B, T)) * 5
        limit = min(T, _schedule(c)[3]) if _reactive(c) else T
        routes = [routes_for(rng, A, inst["depot"][b], inst["task_xy"][b], inst["req"][b], inst["dur"][b], limit) for b in range(B)]
        _inputs[name] = (inst, routes)
    return _inputs[name]


def plain_inputs(name):
    """The case's shape with generate_batch's own durations and synthetic_routes: every task staffed exactly, in ascending order"""
    if name not in _plain:
        from dcmrta_amd.instances import generate_batch, synthetic_routes
        c = CASES[name]
        inst = generate_batch(c["B"], c["A"], c["T"], base_seed=4000 + c["T"])
        _plain[name] = (inst, [synthetic_routes(inst["req"][b], c["A"]) for b in range(c["B"])])
    return _plain[name]


# ------------------------------------------------------------------------------------------------------------------- oracle side
def _oracle(oracle_lib, c, inst, routes, b):
    o = oracle_lib.OracleEnv(c["A"], c["T"]).load(inst["depot"][b], inst["task_xy"][b], inst["req"][b], inst["dur"][b])
    if _reactive(c):
        o.set_visibility(*_schedule(c))
    for a, r in enumerate(routes[b]):
        o.pre_set_route(r, a)
    return o


def _replay(oracle_lib, c, inst, routes):
    """execute_by_route of every env: per env the final() dict plus routes / arrivals / member and abandoned lists"""
    out = []
    for b in range(c["B"]):
        o = _oracle(oracle_lib, c, inst, routes, b)
        ref = o.execute_by_route(_reactive(c))                               # (a TypeError of the reference would raise here)
        ref["routes"] = [o.route(a) for a in range(c["A"])]
        ref["members"] = [o.members(t) for t in range(c["T"])]
        ref["abandoned"] = [o.abandoned(t) for t in range(c["T"])]
        out.append(ref)
    return out


def refs(oracle_lib, name):
    key = CASES[name].get("inputs", name)
    if key not in _refs:
        _refs[key] = _replay(oracle_lib, CASES[key], *inputs(key))
    return _refs[key]


def walk_static(o, req, routes):
    """The static replay through the oracle's primitives (oracle/dcmrta_oracle.c:633-670 without the reactive lines).  Returns one
    entry (task, rule, members before, positions that left) per task and task_update call that removed somebody."""
    T = o.T
    o.set_params(MWT, 100.0)                                                 # :636
    todo = [list(r) if r is not None else [] for r in routes]                # (a None route: the depot action at every decision, :657)
    members = [np.zeros(0, np.int32) for _ in range(T)]
    nab = np.zeros(T, np.int32)
    removals = []

    def task_update():
        o.task_update()
        now_nab = o.final()["n_abandoned"]
        for t in np.flatnonzero(now_nab != nab):
            old, new = members[t], o.members(t)
            left = [j for j, a in enumerate(old) if a not in new]
            assert len(left) == now_nab[t] - nab[t] and len(new) == len(old) - len(left)
            removals.append((int(t), "spread" if req[t] - len(old) <= 0 else "wait", old.copy(), left))      # env/task_env.py:254
            members[t] = new
        nab[:] = now_nab

    finished, guard = False, 0
    while not finished and o.now < CUTOFF:                                   # :639
        ids, t = o.next_decision()                                           # :647
        o.now = t
        task_update()                                                        # :649
        o.agent_update()
        if len(ids) == 0:
            guard += 1
            assert guard <= 8, "the oracle's zero-decider guard would truncate this env"
        else:
            guard = 0
        for a in ids:                                                        # :653
            action = todo[a].pop(0) if todo[a] else 0
            o.agent_step(int(a), action)
            if action:
                members[action - 1] = o.members(action - 1)
            task_update()                                                    # :662
            o.agent_update()
        finished = o.check_finished()                                        # :666
    return removals


def coverage(c, routes, batch, walked):
    """What a batch's final states (and, for a static case, its walked removals) show"""
    A, T = c["A"], c["T"]
    cov = dict(abandonments=0, hi_agents=0, lo_agents=0, chunks=[0] * min((T + 63) // 64, 3), both_chunks=0, twice=0, fin_after=0,
               kept_after=0, top_task=0, most=0, multi=0, nonadjacent=0, slot1=0, spread=0, spread_multi=0)
    for b, ref in enumerate(batch):
        per_agent = np.zeros(A, np.int64)
        top = max(t for r in routes[b] for t in r) - 1              # the highest routed task
        for t, ab in enumerate(ref["abandoned"]):
            if len(ab) == 0:
                continue
            cov["abandonments"] += len(ab)
            cov["hi_agents"] += int((ab >= 64).sum())
            cov["lo_agents"] += int((ab < 64).sum())
            cov["chunks"][min(t // 64, 2)] += len(ab)
            cov["both_chunks"] += bool((ab >= 64).any() and (ab < 64).any())
            cov["fin_after"] += bool(ref["finished"][t])
            cov["kept_after"] += len(ref["members"][t]) > 0
            cov["top_task"] += t == top
            np.add.at(per_agent, ab, 1)
        cov["twice"] += int((per_agent >= 2).sum())
        cov["most"] = max(cov["most"], int(per_agent.max()))
    for env_rem in walked or []:
        for t, rule, old, left in env_rem:
            cov["multi"] += len(left) >= 2
            cov["nonadjacent"] += any(q - p >= 2 for p, q in zip(left, left[1:]))
            cov["slot1"] += any(j >= 1 for j in left)
            cov["spread"] += rule == "spread"
            cov["spread_multi"] += rule == "spread" and len(left) >= 2
    return cov


def golden_spread_calls(oracle_lib, golden_dir):
    """(static comparable cases, removing calls, spread-rule calls) of tests/golden/replay_random.json under walk_static"""
    from fixtures_ref import random_replay_cases
    n_cases = n_calls = n_spread = 0
    for c, inst in random_replay_cases(golden_dir):
        if c["reactive"] or c["status"] != "ok":
            continue
        o = oracle_lib.OracleEnv(c["A"], c["T"]).load(inst["depot"], inst["task_xy"], inst["req"], inst["dur"])
        rem = walk_static(o, inst["req"], c["routes"])
        n_cases += 1
        n_calls += len(rem)
        n_spread += sum(rule == "spread" for _, rule, _, _ in rem)
    return n_cases, n_calls, n_spread


def test_inputs_reach_every_removal_path(oracle_lib, golden_dir):
    """The coverage conditions, from the oracle alone.  Printed per case: the counts of DESIGN.md §5."""
    t0 = time.perf_counter()
    covs = {}
    for name, c in CASES.items():
        if "inputs" in c:
            continue
        inst, routes = inputs(name)
        batch = refs(oracle_lib, name)
        walked = None
        for b, ref in enumerate(batch):                                      # every env: nothing that would leave it out of a comparison
            assert ref["truncated"] == 0 and ref["max_members_seen"] <= 5, (name, b, ref["truncated"], ref["max_members_seen"])
            assert all(r[-1] == 0 and len(r) <= 4 for r in routes[b]), (name, b)
        if not _reactive(c):
            walked = []
            for b, ref in enumerate(batch):
                o = _oracle(oracle_lib, c, inst, routes, b)
                walked.append(walk_static(o, inst["req"][b], routes[b]))
                for t in range(c["T"]):                                      # the walk is the oracle's own replay
                    assert np.array_equal(o.members(t), ref["members"][t]) and np.array_equal(o.abandoned(t), ref["abandoned"][t]), (name, b, t)
                assert sum(len(left) for _, _, _, left in walked[-1]) == ref["n_abandoned"].sum(), (name, b)
        cov = covs[name] = coverage(c, routes, batch, walked)
        print(name, cov)
        assert cov["most"] <= 2, (name, cov)                                 # hence no abandonment-log overflow (AB_CAP = 16) in a replay
        assert cov["abandonments"] >= 1 and cov["kept_after"] >= 1 and cov["twice"] >= 1, (name, cov)
        if c["A"] > 64:
            assert cov["hi_agents"] >= 1 and cov["lo_agents"] >= 1 and cov["both_chunks"] >= 1, (name, cov)
        if c["T"] > 64:
            assert cov["chunks"][0] >= 1 and cov["chunks"][1] >= 1, (name, cov)
        if c["kernel"] == "k_replay" and c["T"] > 128:
            assert cov["chunks"][2] >= 1, (name, cov)
        if walked is not None:
            assert cov["multi"] >= 1 and cov["nonadjacent"] >= 1 and cov["slot1"] >= 1, (name, cov)
            assert cov["spread"] >= 1, (name, cov)                           # the planted one at least
    # over the file: the highest routed task abandons somebody in a k_replay case with T > 128; each kernel finishes a task that
    # abandoned somebody (g70x66 replays f70x66's inputs on k_replay)
    assert any(covs[n]["top_task"] for n, c in CASES.items() if c["kernel"] == "k_replay" and c["T"] > 128 and "inputs" not in c)
    for kernel in ("k_replay_fast", "k_replay"):
        assert any(covs[c.get("inputs", n)]["fin_after"] for n, c in CASES.items() if c["kernel"] == kernel), kernel
    # plain synthetic routes (run 2 of test_state_across_launches): no abandonment at all
    for name in sorted({n for n, _, _ in STATE_RUNS}):
        inst, routes = plain_inputs(name)
        for ref in _replay(oracle_lib, CASES[name], inst, routes):
            assert ref["n_abandoned"].sum() == 0 and ref["truncated"] == 0 and ref["max_members_seen"] <= 5, name
    print("replay_random.json static cases / removing calls / spread-rule calls:", golden_spread_calls(oracle_lib, golden_dir))
    print("coverage test: %.2f s" % (time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------------------------- GPU side
def _new_env(gpu_device, c, inst):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    env = BatchedTaskEnv(c["B"], c["A"], c["T"], device=gpu_device)
    env.load_instances(**inst)
    if c["vis"]:
        env.set_visibility(*c["vis"])
    return env


def _execute(env, c, routes, cap, placement, log_cap):
    """One replay; every output as a numpy array of its own (the handle's summary and log buffers are overwritten by the next run)"""
    env.load_routes(routes, member_cap=cap)
    env.set_replay_placement(placement)
    env.enable_replay_log(cap=log_cap)
    return {k: v.cpu().numpy().copy() for k, v in env.execute_routes(reactive=_reactive(c)).items()}


def _log_cap(batch):
    return max(len(r[0]) for ref in batch for r in ref["routes"]) + 1


def _bits(x):
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _assert_same(a, b, keys, tag):
    for k in keys:
        assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), (tag, k)


def _assert_same_log(a, b, tag):
    _assert_same(a, b, LOG_KEYS, tag)
    valid = np.arange(a["route"].shape[2])[None, None, :] < a["route_len"][:, :, None]
    assert np.array_equal(np.where(valid, a["route"], -2), np.where(valid, b["route"], -2)), (tag, "route")
    assert np.array_equal(np.where(valid, a["arrival"], 0.0).view(np.uint64), np.where(valid, b["arrival"], 0.0).view(np.uint64)), (tag, "arrival")


def _check(out, batch, c, cap, tag):
    """every env of a logged run against the oracle, bit for bit"""
    assert not (out["flags"] & BAD_FLAGS).any(), (tag, out["flags"])
    assert out["members"].shape == (c["B"], c["T"], cap), tag
    for b, ref in enumerate(batch):
        name = f"{tag} env {b}"
        for k in KEYS_EXACT:
            want = np.asarray(ref[k])
            assert np.array_equal(_bits(out[k][b].astype(want.dtype)), _bits(want)), (name, k, np.flatnonzero(out[k][b].astype(want.dtype) != want)[:8])
        sm = out["summary"][b]
        assert sm[3] == ref["makespan"] and sm[0] == -ref["makespan"] and int(sm[1]) == int(ref["finished"].sum()), name
        assert np.array_equal(sm[2:8].view(np.uint64), ref["metrics"].view(np.uint64)), (name, sm[2:8], ref["metrics"])
        n = out["route_len"][b]
        for a, (rt, ra) in enumerate(ref["routes"]):
            assert n[a] == len(rt), (name, "route_len", a)
            assert np.array_equal(out["route"][b, a, :n[a]], rt), (name, "route", a)
            assert np.array_equal(out["arrival"][b, a, :n[a]].view(np.uint64), ra.view(np.uint64)), (name, "arrival", a)
        assert int(n.sum()) == int(out["steps"][b]), name                    # one entry per agent_step
        want = np.full((c["T"], cap), -1, np.int16)
        for t, m in enumerate(ref["members"]):
            want[t, :len(m)] = m
        assert np.array_equal(out["members"][b], want), (name, "members", np.flatnonzero((out["members"][b] != want).any(1))[:8])
        assert np.array_equal(out["n_members"][b], [len(m) for m in ref["members"]]), name
        assert np.array_equal(out["feasible"][b], ref["feasible"]), (name, "feasible")


@pytest.mark.gpu
@pytest.mark.parametrize("name,cap,placement", RUNS)
def test_replay_with_removals_matches_oracle(gpu_device, oracle_lib, name, cap, placement):
    """Parity with the log on (the LOG = true forms), then the same replay without the log (LOG = false): steps, flags, every
    per-task / per-agent output and the summary rows byte-identical."""
    c = CASES[name]
    inst, routes = inputs(name)
    batch = refs(oracle_lib, name)
    tag = f"{name} cap={cap} {placement}"
    env = _new_env(gpu_device, c, inst)
    out = _execute(env, c, routes, cap, placement, _log_cap(batch))
    _check(out, batch, c, cap, tag)
    plain = _execute(env, c, routes, cap, placement, 0)
    assert not set(plain) & {"route", "arrival", "route_len", "members", "feasible"}, tag
    _assert_same(out, plain, ("steps", "flags", "summary") + KEYS_EXACT, tag + " without the log")
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,cap,placement", STATE_RUNS)
def test_state_across_launches(gpu_device, oracle_lib, name, cap, placement):
    """One handle: the removal-heavy routes, then plain instances with synthetic_routes (no abandonment: asserted on the CPU), then the
    first again.  What a replay leaves in the handle's scratch -- abandonment log and counts -- must not reach the next one: run 2 is
    the oracle's, run 3 is run 1 byte for byte.  dcm_execute_routes re-initialises all replay state in the kernel itself and
    dcm_load_routes / dcm_load_instances only replace their inputs: no reset call is needed between the runs."""
    c = CASES[name]
    inst, routes = inputs(name)
    p_inst, p_routes = plain_inputs(name)
    batch = refs(oracle_lib, name)
    if ("plain", name) not in _refs:
        _refs[("plain", name)] = _replay(oracle_lib, c, p_inst, p_routes)
    p_batch = _refs[("plain", name)]
    log_cap = max(_log_cap(batch), _log_cap(p_batch))
    env = _new_env(gpu_device, c, inst)
    first = _execute(env, c, routes, cap, placement, log_cap)
    _check(first, batch, c, cap, f"{name} run 1")
    env.load_instances(**p_inst)
    second = _execute(env, c, p_routes, cap, placement, log_cap)
    _check(second, p_batch, c, cap, f"{name} run 2")
    env.load_instances(**inst)
    third = _execute(env, c, routes, cap, placement, log_cap)
    _assert_same(first, third, ("steps", "flags", "summary") + KEYS_EXACT, f"{name} run 3")
    _assert_same_log(first, third, f"{name} run 3")
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLACEMENT_CASES)
def test_placements_agree(gpu_device, oracle_lib, name):
    """lds / hbm / auto: byte-identical outputs and logs"""
    c = CASES[name]
    inst, routes = inputs(name)
    log_cap = _log_cap(refs(oracle_lib, name))
    outs = {}
    for placement in ("lds", "hbm", "auto"):
        env = _new_env(gpu_device, c, inst)
        outs[placement] = _execute(env, c, routes, 5, placement, log_cap)
        env.close()
    for placement in ("hbm", "auto"):
        _assert_same(outs["lds"], outs[placement], ("steps", "flags", "summary") + KEYS_EXACT, f"{name} {placement}")
        _assert_same_log(outs["lds"], outs[placement], f"{name} {placement}")
