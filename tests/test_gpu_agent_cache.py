"""What agent_update and the agent observation read of an agent's current task (its feasible flag, time_start, time_finish) in the
register-resident kernels (Fast<>), against the oracle, decision by decision.  The file was written for a per-agent cache of those
values (measured slower and not kept: DESIGN.md 4.2); its cases are the ones in which such state goes stale, and they run what
Fast<> does have: the slot minimum / maximum of task_update (nanmin5 / nanmax5), the global-address-space store of the removal path,
the scalar target lane of apply().

Shapes: 256 envs of 6A/3T with requirements drawn from {2, 3}, and 64 envs of 20A/50T.  The oracle is walked with its step-wise API
(the loop of worker.py:45-87, as in test_gpu_member_removal.py; checked here against the oracle's own rollout).  From that walk alone
-- no kernel involved -- the inputs are shown to contain:
  (a) a task becomes feasible while at least two of its members wait at it;
  (b) an agent whose route[-1] is t but who is NOT a member of t at the call that makes t feasible (t dropped it, a group ahead of it
      completed t), observed afterwards -- route[-1] still t -- as a non-leader: its row reads t's time_start;
  (c) a member whose `assigned` flag is set at a later event than the call that made its task feasible;
  (d) a re-join of a task by an agent still listed in it (Q4);
  (e) a return to the depot once every task is feasible.
max_waiting_time and the seeds below were checked with that walk on the CPU.

On the GPU: the lockstep path (k_step_fast, the same Fast<> text; one reload() per decision) against the walk after every decision;
rollout_random stopped and continued with budgets of 1 and of 7 decisions per launch -- reload() in the middle of an episode, with
feasible tasks in progress -- against the general kernel driven the same way; one episodes=3 launch against the oracle; and the
renewing, a greedy and a logging form once each against the launch they must equal."""
import numpy as np
import pytest

import helpers as H

MAX_TIME = 100.0
#                 A,  T,   B, max_waiting_time, instance seed, choice seed, requirements
CASES = {"6A3T": (6, 3, 256, 1.5, 11, 5, (2, 3)),
         "20A50T": (20, 50, 64, 2.0, 7, 3, None)}
AB_CAP = 16          # entries per agent of the abandonment log (csrc/common.hpp)
CONDITIONS = ("a_two_wait", "b_dropped_then_observed", "c_assigned_later", "d_rejoin", "e_returned")

_walks = {}


def instances(name):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    A, T, B, mwt, iseed, cseed, reqs = CASES[name]
    inst = generate_batch(B, A, T, base_seed=iseed)
    if reqs:
        inst["req"] = np.random.default_rng(iseed).choice(np.array(reqs, np.int32), size=(B, T)).astype(np.int32)
    return inst, env_seeds(cseed, 0, B)


def _load(oracle_lib, name, inst, b):
    A, T, _, mwt = CASES[name][:4]
    return oracle_lib.OracleEnv(A, T, max_waiting_time=mwt, max_time=MAX_TIME).load(inst["depot"][b], inst["task_xy"][b], inst["req"][b],
                                                                                 inst["dur"][b])


def walk_episode(o, seed_e):
    """One episode of the oracle through its step-wise API.  Returns (snaps, hits): the state in front of every decision, and how often
    each of CONDITIONS occurred."""
    from dcmrta_amd.choice import below, draw
    A, T = o.A, o.T
    members = [np.zeros(0, np.int32) for _ in range(T)]
    cur = np.full(A, -2, np.int32)                       # route[-1] (-2: no route yet, -1: the depot), kept here, checked at the end
    for a in range(A):
        r = o.route(a, 64)[0]
        cur[a] = r[-1] if len(r) else -2
    hits = dict.fromkeys(CONDITIONS, 0)
    snaps, state = [], dict(feasible=np.zeros(T, np.uint8), returned=np.zeros(A, np.uint8))
    pend_b, pend_c = set(), set()                        # (agent, task[, now of the call]) waiting for their later observation

    def updates():
        """task_update + agent_update (worker.py:50-51 / :74-76) and what they show"""
        was_f, was_r = state["feasible"].copy(), state["returned"].copy()
        o.task_update()
        f = o.final()
        for t in range(T):
            members[t] = o.members(t) if f["n_members"][t] != len(members[t]) or f["feasible"][t] != was_f[t] else members[t]
        o.agent_update()
        assigned = o.agent_status(0)[:, 5]
        for a, t, now0 in list(pend_c):                  # (c): still on t, assigned now, at a later event
            if cur[a] != t:
                pend_c.discard((a, t, now0))
            elif assigned[a] == 1.0 and o.now > now0:
                hits["c_assigned_later"] += 1
                pend_c.discard((a, t, now0))
        for t in np.flatnonzero((f["feasible"] != 0) & (was_f == 0)):
            mem = set(int(m) for m in members[t])
            arrived = [a for a in mem if cur[a] == t and o.route(a, 512)[1][-1] < o.now]
            hits["a_two_wait"] += len(arrived) >= 2
            pend_b.update((a, int(t)) for a in range(A) if cur[a] == t and a not in mem)
            pend_c.update((a, int(t), o.now) for a in mem if cur[a] == t and assigned[a] == 0.0)
        if f["feasible"].all() and (f["returned"] != 0).sum() > (was_r != 0).sum():
            hits["e_returned"] += 1
        state.update(f)
        state["assigned"] = assigned

    finished, d, empty = False, 0, 0
    while not finished and o.now < MAX_TIME:                               # worker.py:45
        ids, t = o.next_decision()                                         # :47
        groups = o.get_unique_group(ids) if len(ids) else []              # :48
        o.now = t                                                          # :49
        updates()                                                          # :50-51
        if not groups:
            empty += 1
            if empty > 4:
                break
        else:
            empty = 0
        for group in groups:                                               # :52
            while group:                                                   # :53
                leader = group[below(draw(seed_e, d, 0), len(group))]      # :54
                mask, ag, tk = o.mask(), o.agent_status(leader), o.task_status(leader)
                for a, t in list(pend_b):                                  # (b): still on t, seen by somebody else's decision
                    if cur[a] != t:
                        pend_b.discard((a, t))
                    elif leader != a:
                        hits["b_dropped_then_observed"] += 1
                        pend_b.discard((a, t))
                snaps.append(dict(leader=leader, now=o.now, mask=mask, agents_obs=ag, tasks_obs=tk, current=cur.copy(),
                                  assigned=state["assigned"].astype(np.uint8), returned=state["returned"].copy()))
                action = H.host_random_action(mask, seed_e, d)
                snaps[-1]["action"] = action
                vacancy = int(tk[action, 0]) if action >= 1 else len(group)            # :327 (the status may be stale)
                group.remove(leader)                                       # :328
                step = [leader]
                if vacancy > 1:                                            # :330-333
                    for j in range(min(vacancy - 1, len(group))):
                        step.append(group.pop(below(draw(seed_e, d, 2 + j), len(group))))
                for m in step:
                    if action >= 1 and m in members[action - 1]:
                        hits["d_rejoin"] += 1                              # Q4 :321-322
                    o.agent_step(m, action)                                # :338-340
                    cur[m] = action - 1
                if action >= 1:
                    members[action - 1] = o.members(action - 1)
                updates()                                                  # :74-76
                d += 1
        finished = o.check_finished()                                      # :85
    for a in range(A):
        r = o.route(a, 512)[0]
        assert cur[a] == (r[-1] if len(r) else -2), ("route[-1] as the walk kept it", a)
    return snaps, hits


def walks(oracle_lib, name):
    """(instances, seeds, per-env snapshots, the batch's hits, the oracle's own three episodes): computed once, read-only afterwards"""
    if name not in _walks:
        inst, seeds = instances(name)
        B = CASES[name][2]
        snaps, eps, total = [], [], dict.fromkeys(CONDITIONS, 0)
        for b in range(B):
            s, h = walk_episode(_load(oracle_lib, name, inst, b), int(seeds[b]))
            snaps.append(s)
            for k in total:
                total[k] += h[k]
            three, d0 = [], 0
            for ep in range(3):
                three.append(_load(oracle_lib, name, inst, b).rollout(int(seeds[b]), d0, oracle_lib.POLICY_RANDOM, cap_steps=20000,
                                                                     record=(ep == 0)))
                d0 += three[-1]["n_steps"]
            eps.append(three)
        _walks[name] = (inst, seeds, snaps, total, eps)
    return _walks[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_walk_is_the_oracles_episode(oracle_lib, name):
    """The step-wise loop above against the oracle's own rollout of the first episode: every decision's record"""
    _, _, snaps, _, eps = walks(oracle_lib, name)
    for b, (s, three) in enumerate(zip(snaps, eps)):
        r = three[0]
        assert len(s) == r["n_steps"], (name, b)
        for k in ("leader", "action", "now", "mask", "agents_obs", "tasks_obs"):
            assert np.array_equal(np.array([x[k] for x in s]).reshape(r[k].shape), r[k]), (name, b, k)


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_show_every_case_of_the_cache(oracle_lib, name):
    """The coverage conditions (a) - (e), from the oracle alone, in each of the two batches"""
    hits = walks(oracle_lib, name)[3]
    print(name, hits)
    for k in CONDITIONS:
        assert hits[k] >= 1, (name, k, hits)


def _env(gpu_device, name, inst, **kw):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    A, T, B, mwt = CASES[name][:4]
    return BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=mwt, **kw).load_instances(**inst)


def _records(env):
    """The envs' records, u8[B, record_bytes]: the head of clone_state().  Behind them clone_state() holds the abandonment side tables,
    which are NOT compared byte for byte: a log row is in event order, and when two tasks drop the same agent in ONE task_update call
    the general kernel appends in the order its task lanes' atomics land while Fast<> walks the dropping tasks in ascending order (the
    reference's).  Every reader sorts the row by task id or counts it (terminal metrics, dcm_get_abandoned), so the order inside a call
    is not part of the state; the abandonments are compared as abandoned_counts().  (Seen here: 20A/50T env 53, agent 5, tasks 30 and
    33 in one call at decision 154.)"""
    blob = env.clone_state().cpu().numpy()
    side = env.B * (env.A * AB_CAP * 2 + (2 * env.A * env.T + 15) // 16 * 16)     # the logs of all envs, then their overflow counts
    n, rest = divmod(blob.size - side, env.B)
    assert rest == 0 and n >= env.record_bytes(), (blob.size, side, env.record_bytes())
    return blob[:env.B * n].reshape(env.B, n)


def _general_rollout(env, policy, episodes, budgets=None):
    """The same launch on the GENERAL kernel (k_rollout_random keeps the record in LDS and gathers what the cache holds): a launch that
    is given some but not all of the observation buffers takes it (plan.hpp, rollout_kind)."""
    import torch
    from dcmrta_amd._lib import check
    from dcmrta_amd.batched_env import _ptr
    steps = torch.empty((env.B,), dtype=torch.int64, device=env.device)
    per_env = None if budgets is None else env._dev(budgets, torch.int64)
    with torch.cuda.device(env.device):
        check(env._lib.dcm_rollout_policy(env._h, env.POLICIES[policy], int(episodes), -1, _ptr(per_env),
                                          _ptr(env._agents), None, None, _ptr(steps), env._stream()))
    return steps


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_lockstep_after_every_decision(gpu_device, oracle_lib, name):
    """k_step_fast against the walk: both observation tensors and the mask bit for bit, the event time, the agents' flags"""
    import torch
    A, T, B = CASES[name][:3]
    inst, seeds, snaps, _, eps = walks(oracle_lib, name)
    env = _env(gpu_device, name, inst)
    obs = env.reset(seeds)
    count = np.zeros(B, np.int64)
    for _ in range(max(len(s) for s in snaps) + 1):
        active = obs.active.cpu().numpy().astype(bool)
        assert np.array_equal(active, count < np.array([len(s) for s in snaps])), (name, count)
        if not active.any():
            break
        ag, tk, mk, ld = (x.cpu().numpy() for x in (obs.agents, obs.tasks, obs.mask, obs.leader))
        now = env.status()["now"].cpu().numpy()
        st = {k: v.cpu().numpy() for k, v in env.agents_state().items()}
        actions = np.zeros(B, np.int32)
        for b in np.flatnonzero(active):
            s = snaps[b][count[b]]
            tag = f"{name} env {b} decision {count[b]}"
            assert int(ld[b]) == s["leader"] and now[b] == s["now"], tag
            assert np.array_equal(mk[b].astype(np.uint8), s["mask"]), (tag, "mask")
            assert np.array_equal(ag[b].view(np.uint32), s["agents_obs"].view(np.uint32)), (tag, "agent observation", ag[b], s["agents_obs"])
            assert np.array_equal(tk[b].view(np.uint32), s["tasks_obs"].view(np.uint32)), (tag, "task observation")
            for k in ("current", "assigned", "returned"):
                assert np.array_equal(st[k][b].astype(s[k].dtype), s[k]), (tag, k, st[k][b], s[k])
            actions[b] = s["action"]
            count[b] += 1
        obs = env.step(torch.from_numpy(actions).to(gpu_device))
    else:
        raise AssertionError("the lockstep loop did not end")
    sm = env.summary().cpu().numpy()
    for b in range(B):
        r = eps[b][0]
        assert sm[b, 0] == r["reward"] and int(sm[b, 1]) == int(r["finished"].sum()), (name, b)
        assert np.array_equal(sm[b, 2:8], r["metrics"]), (name, b, sm[b], r["metrics"])
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [1, 7])
@pytest.mark.parametrize("name", list(CASES))
def test_stopped_and_continued_launches(gpu_device, oracle_lib, name, budget):
    """rollout_random with `budget` decisions per launch through the first episode, beside the general kernel driven the same way:
    after every launch the steps, the observation of the last decision taken (against the walk), and the records byte for byte"""
    B = CASES[name][2]
    inst, seeds, snaps, _, eps = walks(oracle_lib, name)
    n = np.array([len(s) for s in snaps])
    fast, gen = _env(gpu_device, name, inst), _env(gpu_device, name, inst)
    fast.reset(seeds, observe=False); gen.reset(seeds, observe=False)
    done = np.zeros(B, np.int64)
    for launch in range((int(n.max()) + budget - 1) // budget):
        want = np.minimum(budget, n - done)                          # (per env: a finished env would start its next episode)
        sf = fast.rollout_random(episodes=1, max_decisions=want).cpu().numpy()
        sg = _general_rollout(gen, "random", 1, want).cpu().numpy()
        assert np.array_equal(sf, want) and np.array_equal(sg, want), (name, budget, launch)
        done += want
        o = fast.obs()
        ag, tk, mk = (x.cpu().numpy() for x in (o.agents, o.tasks, o.mask))
        for b in np.flatnonzero(want > 0):
            s = snaps[b][done[b] - 1]
            tag = f"{name} budget {budget} launch {launch} env {b}"
            assert np.array_equal(mk[b].astype(np.uint8), s["mask"]), (tag, "mask")
            assert np.array_equal(ag[b].view(np.uint32), s["agents_obs"].view(np.uint32)), (tag, "agent observation")
            assert np.array_equal(tk[b].view(np.uint32), s["tasks_obs"].view(np.uint32)), (tag, "task observation")
        rf, rg = _records(fast), _records(gen)
        bad = np.argwhere(rf != rg)
        assert len(bad) == 0, (name, budget, launch, "records: (env, byte) that differ", bad[:16].tolist())
        assert np.array_equal(fast.abandoned_counts().cpu().numpy(), gen.abandoned_counts().cpu().numpy()), (name, budget, launch, "abandonments")
    assert np.array_equal(done, n)
    sm = fast.summary().cpu().numpy()
    assert np.array_equal(sm.view(np.uint64), gen.summary().cpu().numpy().view(np.uint64)), (name, budget)
    for b, three in enumerate(eps):
        assert sm[b, 0] == three[0]["reward"] and np.array_equal(sm[b, 2:8], three[0]["metrics"]), (name, budget, b)
    fast.close(); gen.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_three_episodes_in_one_launch(gpu_device, oracle_lib, name):
    B = CASES[name][2]
    inst, seeds, _, _, eps = walks(oracle_lib, name)
    env = _env(gpu_device, name, inst)
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=3).cpu().numpy()
    got, sm = ring.cpu().numpy(), env.summary().cpu().numpy()
    assert np.array_equal(steps, np.array([sum(r["n_steps"] for r in three) for three in eps])), name
    for b, three in enumerate(eps):
        assert [got[b, i] for i in range(3)] == [r["reward"] for r in three], (name, b)
        last = three[2]
        assert sm[b, 0] == last["reward"] and int(sm[b, 1]) == int(last["finished"].sum()), (name, b)
        assert np.array_equal(sm[b, 2:8], last["metrics"]), (name, b, sm[b], last["metrics"])
    env.close()


def _results(env, steps, ring, whole_state):
    o = env.obs()
    state = env.clone_state().cpu().numpy() if whole_state else _records(env)      # (see _records: the log rows' order)
    return ([x.cpu().numpy().copy() for x in (steps, env.summary(), ring, env.abandoned_counts())] + [state.copy()],
            [x.cpu().numpy().copy() for x in (o.agents, o.tasks, o.mask)])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["logging", "greedy", "renewing"])
def test_the_other_forms_equal_the_launches_they_equal_today(gpu_device, oracle_lib, form):
    """The kernel forms that compile the same Fast<> text, two episodes of the 20A/50T batch each:
    logging (k_lg_rollout_fast, random policy)  == the plain launch (k_rollout_fast): everything, the observation buffers included;
    greedy  (k_hp_rollout_fast, "first")         == the general kernel under the same policy: steps, records, summary rows, returns;
    renewing (k_rn_rollout_fast)                 == the general kernel's renewing form on the same generated instances: the same."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    name = "20A50T"
    A, T, B, mwt = CASES[name][:4]
    inst, seeds = walks(oracle_lib, name)[:2]

    def make():
        if form != "renewing":
            return _env(gpu_device, name, inst)
        env = BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=mwt)
        env.generate_instances(np.arange(5100, 5100 + B, dtype=np.uint64))
        env.set_instance_renewal(B)
        return env
    out = []
    for ref in (True, False):
        env = make()
        ring = env.enable_return_log(2)
        if form == "logging" and not ref:
            env.enable_rollout_log(64)
        env.reset(seeds, observe=False)
        if form == "logging":
            steps = env.rollout("random", episodes=2)
        elif ref:
            steps = _general_rollout(env, "first" if form == "greedy" else "random", 2)
        else:
            steps = env.rollout("first" if form == "greedy" else "random", episodes=2)
        out.append(_results(env, steps, ring, whole_state=(form == "logging")))     # the same kernel family: side tables too
        if form == "renewing":
            assert (env.instance_index().cpu().numpy() == 1).all()
        env.close()
    assert int(out[0][0][0].sum()) > 0
    for i, (a, b) in enumerate(zip(out[0][0], out[1][0])):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (form, i)
    if form == "logging":
        for i, (a, b) in enumerate(zip(out[0][1], out[1][1])):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (form, "observation", i)
