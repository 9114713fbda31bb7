"""Member removal of the kernels that test_gpu_member_removal.py does not reach: FastG<NAC,NTC>::tu_chunk (csrc/rollout_fast_g.hpp: the
five-slot compaction with its idl / idh id split, the per-agent-chunk `gone` masks, the abandonment log and its overflow table, the
incremental chunk visiting), FastMc (csrc/rollout_fast_mc.hpp), Sim<...>::task_update_one of the general kernels, and the wide form
with sixteen member slots -- against the oracle, decision by decision.

max_waiting_time is short in every case, so both removal rules fire all the time.  The oracle is walked with walk_episode of
removal_ref.py (checked in walks() against the oracle's own rollout), and from that walk alone -- no kernel involved --
test_inputs_reach_every_removal_path shows that the inputs hold what each kernel can get wrong: a removal at every slot of a full list
(slot 4 is the idh word), removals in every task chunk, of agents of the second agent chunk, of both agent chunks by one task, and agents
abandoned more than AB_CAP = 16 times in an episode (the overflow table, also in a ragged env whose own T is below the layout's).

On the GPU: k_step in lockstep after every decision, the persistent kernels stopped by decision budgets (after every decision where
the budget is 1) with the state they wrote back, and three episodes in one launch (the log and the table are cleared at a restart)."""
import numpy as np
import pytest

import helpers as H
import oracle_ref as O
from removal_ref import Lists, assert_obs, assert_state, coverage, walk_episode

AB_CAP = 16                 # entries of an agent's abandonment log (csrc/common.hpp); further ones go to the count table
INST_SEED, CHOICE_SEED = 11, 5
RAGGED_SIZES = ((70, 130), (64, 64), (65, 128), (64, 129), (70, 65), (1, 130), (20, 66), (66, 127))

# req: None = as generated (1..5), a tuple = drawn from it, an int = drawn from 1..that (wide).  kernel / chunks: what
# rollout_random launches, <NAC,NTC> of FastG.  sim: the Sim<> instantiation behind k_step (and behind k_rollout_random).
# lockstep: None = not run, 0 = every decision, n = the first n decisions of every env.  budget: largest per-launch decision budget.
CASES = {
    "g2x2": dict(A=70, T=66, B=8, mwt=1.5, req=(3, 4, 5), kernel="k_rollout_fast_g", chunks=(2, 2), sim="<128,256,true>", lockstep=0, budget=1),
    "g2x3": dict(A=70, T=130, B=4, mwt=1.0, req=None, kernel="k_rollout_fast_g", chunks=(2, 3), sim="<128,256,true>", lockstep=None, budget=8),
    "g1x4": dict(A=40, T=200, B=4, mwt=1.5, req=(3, 4, 5), kernel="k_rollout_fast_g", chunks=(1, 4), sim="<128,256,true>", lockstep=None, budget=8),
    "g2x4": dict(A=128, T=256, B=2, mwt=1.0, req=None, kernel="k_rollout_fast_g", chunks=(2, 4), sim="<128,256,true>", lockstep=None, budget=8),
    "mc": dict(A=50, T=200, B=4, mwt=1.5, req=(3, 4, 5), kernel="k_rollout_fast_mc", chunks=None, sim="<50,200,false>", lockstep=300, budget=8),
    "rt": dict(A=100, T=300, B=2, mwt=2.0, req=None, kernel="k_rollout_random", chunks=None, sim="<0,0,false>", lockstep=300, budget=8),
    "wide": dict(A=24, T=9, B=16, mwt=2.0, req=16, kernel="k_rollout_random", chunks=None, sim="<0,0,false,16>", lockstep=0, budget=1, member_cap=16),
    "ragged": dict(A=70, T=130, B=8, mwt=1.0, req=None, kernel="k_rollout_fast_g", chunks=(2, 3), sim="<128,256,true>", lockstep=0, budget=1,
                   sizes=RAGGED_SIZES),
}
FAST_G = [n for n, c in CASES.items() if c["kernel"] == "k_rollout_fast_g" and "sizes" not in c]
RENEW = dict(CASES["g2x2"], base=8500)          # g2x2's shape on generated instances, a new one at every restart

_walks, _first, _renew = {}, {}, {}


def test_cases_run_the_kernels_they_name():
    """roofline.rollout_kernel_name (pinned to csrc/plan.hpp by test_host.py) and the two chunk rules of plan.hpp, restated"""
    from dcmrta_amd.roofline import rollout_kernel_name, step_kernel_name
    for name, c in CASES.items():
        A, T = c["A"], c["T"]
        # a wide handle takes the general kernels whatever its shape (plan::rollout_kind; test_host.py asks plan.hpp itself)
        assert ("k_rollout_random" if c.get("member_cap", 5) > 5 else rollout_kernel_name(A, T)) == c["kernel"], name
        assert c.get("member_cap", 5) > 5 or step_kernel_name(A, T) == "k_step", name
        if c["chunks"]:
            assert (2 if A > 64 else 1, 4 if T > 192 else 3 if T > 128 else 2) == c["chunks"], name      # plan::fast_g_*_chunks
    assert {CASES[n]["chunks"] for n in FAST_G} == {(2, 2), (2, 3), (1, 4), (2, 4)}
    assert len(RAGGED_SIZES) == CASES["ragged"]["B"] and RENEW["kernel"] == "k_rollout_fast_g"


def sizes(name, b):
    c = CASES[name]
    return c["sizes"][b] if "sizes" in c else (c["A"], c["T"])


def instances(name):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    c = CASES[name]
    B, A, T = c["B"], c["A"], c["T"]
    inst = generate_batch(B, A, T, base_seed=INST_SEED)
    rng = np.random.default_rng(INST_SEED)
    if isinstance(c["req"], tuple):
        inst["req"] = rng.choice(np.array(c["req"], np.int32), size=(B, T)).astype(np.int32)
    elif c["req"]:
        inst["req"] = rng.integers(1, c["req"] + 1, (B, T)).astype(np.int32)
    if "sizes" in c:
        inst["n_agents"] = np.array([s[0] for s in c["sizes"]], np.int32)
        inst["n_tasks"] = np.array([s[1] for s in c["sizes"]], np.int32)
    return inst, env_seeds(CHOICE_SEED, 0, B)


def _load(oracle_lib, name, inst, b):
    a, t = sizes(name, b)
    return oracle_lib.OracleEnv(a, t, max_waiting_time=CASES[name]["mwt"]).load(inst["depot"][b], inst["task_xy"][b, :t], inst["req"][b, :t],
                                                                              inst["dur"][b, :t])


def walks(oracle_lib, name):
    """(instances, seeds, per-env snapshots, per-env removals, the oracle's own three episodes): computed once, read-only afterwards.
    The walk is checked against the oracle's rollout of the first episode here, every decision's record; the snapshots then keep the
    abandonment counts as (flat indices, values) of the non-zero entries, not as a dense table per decision."""
    if name not in _walks:
        inst, seeds = instances(name)
        snaps, rem, eps = [], [], []
        for b in range(CASES[name]["B"]):
            s, r = walk_episode(_load(oracle_lib, name, inst, b), inst["req"][b], int(seeds[b]))
            three = O.episodes_first_recorded(*sizes(name, b), O.one(inst, b, sizes(name, b)[1]), seeds[b], "random", 3, CASES[name]["mwt"])
            first = three[0]
            assert len(s) == first["n_steps"], (name, b)
            for k in ("leader", "action", "now", "mask", "agents_obs", "tasks_obs"):
                assert np.array_equal(np.array([x[k] for x in s]).reshape(first[k].shape), first.pop(k)), (name, b, k)
            for x in s:
                ab = x.pop("abandoned")
                idx = np.flatnonzero(ab)
                x["abandoned"] = (idx, ab.ravel()[idx].astype(np.int16))
            snaps.append(s); rem.append(r); eps.append(three)
        _walks[name] = (inst, seeds, snaps, rem, eps)
    return _walks[name]


def chunk_coverage(rem, n_tasks):
    """What the removals of a batch show beyond coverage(): positions that left a list of any length, the longest list that lost a
    member, removing calls per task chunk, removals of agents of the second chunk (id >= 64), tasks that removed agents of both
    chunks in one call, and per env the largest number of abandonments of one agent."""
    slots, longest, hi, both = set(), 0, 0, 0
    per_chunk = np.zeros((max(n_tasks) + 63) // 64, np.int64)
    most = []
    for env_rem in rem:
        per_agent = {}
        for t, rule, old, left in env_rem:
            slots.update(left)
            longest = max(longest, len(old))
            per_chunk[t // 64] += 1
            gone = [int(old[j]) for j in left]
            hi += sum(a >= 64 for a in gone)
            both += any(a >= 64 for a in gone) and any(a < 64 for a in gone)
            for a in gone:
                per_agent[a] = per_agent.get(a, 0) + 1
        most.append(max(per_agent.values(), default=0))
    return dict(slots=slots, longest=longest, per_chunk=per_chunk.tolist(), hi_agents=hi, both_chunks=both, most_per_agent=most)


def _merge(covs):
    out = dict(slots5=set(), wait_skip=0, spread_multi=0, two_tasks=0, calls=0)
    for c in covs:
        out["slots5"] |= c["slots5"]
        for k in ("wait_skip", "spread_multi", "two_tasks", "calls"):
            out[k] += c[k]
    return out


def test_inputs_reach_every_removal_path(oracle_lib):
    """The coverage conditions, from the oracle alone"""
    cov, ext = {}, {}
    for name in CASES:
        rem = walks(oracle_lib, name)[3]
        cov[name] = coverage(rem)
        ext[name] = chunk_coverage(rem, [sizes(name, b)[1] for b in range(CASES[name]["B"])])
        print(name, cov[name], ext[name])
    for name in FAST_G + ["rt"]:                                   # a removing call in every task chunk the shape has
        n_chunks = (CASES[name]["T"] + 63) // 64
        assert len(ext[name]["per_chunk"]) == n_chunks and min(ext[name]["per_chunk"]) >= 1, (name, ext[name])
    for name, c in CASES.items():
        if c["A"] > 64:                                            # the second agent chunk, and one task removing from both chunks
            assert ext[name]["hi_agents"] >= 1 and ext[name]["both_chunks"] >= 1, (name, ext[name])
    for who, c in (("FastG", _merge(cov[n] for n in FAST_G)), ("mc", cov["mc"]), ("rt", cov["rt"])):
        assert c["slots5"] == {0, 1, 2, 3, 4}, (who, c)            # a removal at every slot of a five-member list (4: the idh word)
        assert c["spread_multi"] >= 1 and c["wait_skip"] >= 1 and c["two_tasks"] >= 1, (who, c)
    assert ext["wide"]["slots"] == set(range(16)) and ext["wide"]["longest"] == 16, ext["wide"]
    assert cov["wide"]["spread_multi"] >= 1 and cov["wide"]["wait_skip"] >= 1 and cov["wide"]["two_tasks"] >= 1, cov["wide"]
    # the abandonment log overflows: one agent is abandoned more than AB_CAP times in an episode
    assert any(max(ext[n]["most_per_agent"]) > AB_CAP for n in FAST_G if CASES[n]["A"] > 64), ext
    for name in ("mc", "rt", "wide", "ragged"):
        assert max(ext[name]["most_per_agent"]) > AB_CAP, (name, ext[name])
    # ragged: the overflow in an env whose own T is below the layout's (the table is indexed with T_e), a removal in an env of one agent chunk
    rem, T = walks(oracle_lib, "ragged")[3], CASES["ragged"]["T"]
    assert any(m > AB_CAP for m, (a, t) in zip(ext["ragged"]["most_per_agent"], RAGGED_SIZES) if t < T), ext["ragged"]
    assert any(len(r) for r, (a, t) in zip(rem, RAGGED_SIZES) if a <= 64)


# ------------------------------------------------------------------------------------------------------------------- GPU side
def _env(gpu_device, name, inst):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    c = CASES[name]
    return BatchedTaskEnv(c["B"], c["A"], c["T"], device=gpu_device, max_waiting_time=c["mwt"], member_cap=c.get("member_cap", 5)) \
        .load_instances(**inst)


def _state(env):
    return (env.task_members().cpu().numpy(), env.abandoned_counts().cpu().numpy(), {k: v.cpu().numpy() for k, v in env.tasks_state().items()})


def _assert_final(env, name, eps):
    fin = H.gpu_final(env)
    for b, three in enumerate(eps):
        a, t = sizes(name, b)
        got = dict(fin[b])
        for k in H.FINAL_EXACT:
            got[k] = fin[b][k][:a] if k in ("travel_dist", "returned", "agent_wait") else fin[b][k][:t]
        H.assert_final_matches(got, three[0], f"{name} env {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["lockstep"] is not None])
def test_lockstep_after_every_decision(gpu_device, oracle_lib, name):
    """k_step (Sim<...>::task_update_one) against the walk: the state and the observation in front of every decision -- of the
    first `lockstep` decisions where the case says so; the episode is stepped to its end in any case -- and the end state."""
    import torch
    c = CASES[name]
    B, T, limit = c["B"], c["T"], c["lockstep"] or 1 << 30
    inst, seeds, snaps, _, eps = walks(oracle_lib, name)
    n = np.array([len(s) for s in snaps])
    lists = [Lists(sizes(name, b)[1], c.get("member_cap", 5)) for b in range(B)]
    env = _env(gpu_device, name, inst)
    obs = env.reset(seeds)
    count = np.zeros(B, np.int64)
    for _ in range(int(n.max()) + 1):
        active = obs.active.cpu().numpy().astype(bool)
        assert np.array_equal(active, count < n), (name, count)
        if not active.any():
            break
        check = np.flatnonzero(active & (count < limit))
        if len(check):
            ag, tk, mk, ld = (x.cpu().numpy() for x in (obs.agents, obs.tasks, obs.mask, obs.leader))
            now = env.status()["now"].cpu().numpy()
            mem, abc, ts = _state(env)
        actions = np.zeros(B, np.int32)
        for b in np.flatnonzero(active):
            actions[b] = snaps[b][count[b]]["action"]
        for b in check:
            s = snaps[b][count[b]]
            tag = f"{name} env {b} decision {count[b]}"
            a, t = sizes(name, b)
            assert int(ld[b]) == s["leader"] and now[b] == s["now"], (tag, "leader / now")
            assert_state(tag, s, lists[b], a, t, mem[b], abc[b, :a, :t], {k: v[b] for k, v in ts.items()})
            assert not abc[b, a:].any() and not abc[b, :, t:].any(), (tag, "abandonment counts beyond the env's sizes")
            assert_obs(tag, s, a, t, ag[b], tk[b], mk[b])
        count += active
        obs = env.step(torch.from_numpy(actions).to(gpu_device))
    else:
        raise AssertionError("the lockstep loop did not end")
    sm = env.summary().cpu().numpy()
    for b in range(B):
        O.assert_summary(sm[b], eps[b][0], (name, b))
    _assert_final(env, name, eps)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_persistent_kernel_under_decision_budgets(gpu_device, oracle_lib, name):
    """rollout_random(episodes=1, max_decisions=budget[B]) launch after launch.  After every launch the state the kernel wrote back is
    the walk's snapshot in front of the next decision, observe() of it included, and the stored observation is the oracle's record of
    the last decision taken.  Budget 1: a stop after every decision of the episode; otherwise per-env budgets drawn from 1..8."""
    c = CASES[name]
    B, top = c["B"], c["budget"]
    inst, seeds, snaps, _, eps = walks(oracle_lib, name)
    n = np.array([len(s) for s in snaps], np.int64)
    lists = [Lists(sizes(name, b)[1], c.get("member_cap", 5)) for b in range(B)]
    rng = np.random.default_rng(c["A"] * 1000 + c["T"])
    env = _env(gpu_device, name, inst)
    env.reset(seeds, observe=False)
    taken = np.zeros(B, np.int64)
    for launch in range(int(n.max()) + 1):
        if (taken >= n).all():
            break
        budget = np.where(taken < n, rng.integers(1, top + 1, B), 0).astype(np.int64)   # finished envs: 0, they must not start another episode
        steps = env.rollout_random(episodes=1, max_decisions=budget).cpu().numpy()
        assert np.array_equal(steps, np.minimum(budget, n - taken)), (name, launch, steps, budget, n - taken)
        ran = budget > 0
        taken += steps
        stored = env.obs()
        ag, tk, mk = (x.cpu().numpy() for x in (stored.agents, stored.tasks, stored.mask))   # the kernel's own stores: read before observe()
        for b in np.flatnonzero(ran):
            assert_obs(f"{name} env {b}: stored observation of decision {taken[b] - 1}", snaps[b][taken[b] - 1], *sizes(name, b), ag[b], tk[b], mk[b])
        mem, abc, ts = _state(env)
        st = {k: v.cpu().numpy() for k, v in env.status().items()}
        o2 = env.observe()
        ag, tk, mk, ld, act = (x.cpu().numpy() for x in (o2.agents, o2.tasks, o2.mask, o2.leader, o2.active))
        for b in np.flatnonzero(ran):
            tag = f"{name} env {b} launch {launch}: state in front of decision {taken[b]}"
            assert st["decisions"][b] == taken[b], tag
            if taken[b] >= n[b]:
                assert not act[b] and (st["flags"][b] & 1), (tag, "the episode must be over")
                continue
            s = snaps[b][taken[b]]
            a, t = sizes(name, b)
            assert act[b] and int(ld[b]) == s["leader"] and st["now"][b] == s["now"], (tag, "leader / now")
            assert_state(tag, s, lists[b], a, t, mem[b], abc[b, :a, :t], {k: v[b] for k, v in ts.items()})
            assert not abc[b, a:].any() and not abc[b, :, t:].any(), (tag, "abandonment counts beyond the env's sizes")
            assert_obs(tag, s, a, t, ag[b], tk[b], mk[b])
    else:
        raise AssertionError("the episodes did not end")
    _assert_final(env, name, eps)
    env.close()


def _assert_three(name, steps, ring, sm, eps):
    assert np.array_equal(steps, np.array([sum(r["n_steps"] for r in three) for three in eps])), (name, steps)
    for b, three in enumerate(eps):
        assert [ring[b, i] for i in range(3)] == [r["reward"] for r in three], (name, b)
        O.assert_summary(sm[b], three[2], (name, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_three_episodes_in_one_launch(gpu_device, oracle_lib, name):
    """steps, the three returns and summary() bit for bit: the log and the overflow table of an episode that overflowed are cleared"""
    inst, seeds, _, _, eps = walks(oracle_lib, name)
    env = _env(gpu_device, name, inst)
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=3).cpu().numpy()
    _assert_three(name, steps, ring.cpu().numpy(), env.summary().cpu().numpy(), eps)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g2x2", "mc"])
def test_three_greedy_episodes_in_one_launch(gpu_device, oracle_lib, name):
    """rollout("first"): the general form of the greedy kernels at these shapes, against the oracle under POLICY_FIRST"""
    inst, seeds = instances(name)
    if name not in _first:
        _first[name] = [O.episodes(*sizes(name, b), O.one(inst, b, sizes(name, b)[1]), seeds[b], "first", 3, CASES[name]["mwt"])
                        for b in range(CASES[name]["B"])]
    env = _env(gpu_device, name, inst)
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    steps = env.rollout("first", episodes=3).cpu().numpy()
    _assert_three(name, steps, ring.cpu().numpy(), env.summary().cpu().numpy(), _first[name])
    env.close()


@pytest.mark.gpu
def test_three_episodes_on_renewed_instances(gpu_device, oracle_lib):
    """g2x2's shape with set_instance_renewal(B): episode k of env b plays the instance of instances.renewal_seeds(base + b, k, B)"""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_instance, renewal_seeds
    c = RENEW
    B, A, T = c["B"], c["A"], c["T"]
    seeds = env_seeds(CHOICE_SEED, 0, B)

    if not _renew:
        _renew["eps"] = [O.episodes(A, T, lambda k: generate_instance(A, T, int(renewal_seeds(c["base"] + b, k, B))), seeds[b], "random", 3, c["mwt"])
                         for b in range(B)]
    env = BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=c["mwt"])
    env.generate_instances(c["base"])
    env.set_instance_renewal(B)
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=3).cpu().numpy()
    _assert_three("renew", steps, ring.cpu().numpy(), env.summary().cpu().numpy(), _renew["eps"])
    assert np.array_equal(env.instance_index().cpu().numpy(), np.full(B, 2))
    env.close()
