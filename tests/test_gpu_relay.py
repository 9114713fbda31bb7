"""One episode handed from kernel family to kernel family.  Every entry point picks its own kernel (csrc/plan.hpp), every kernel has a
head that loads the HBM record and a tail that writes it back, and include/dcmrta_env.h promises that they meet in that record: any
entry point carries on from a budget stop or a dcm_step with identical results.  The other test files stop and continue a family with
itself; here every ordered pair of the families a shape has is one handover, and after every leg the handle is compared with the
oracle's walk of the episode (removal_ref.assert_handover), bit for bit.

  1. the state relay, random policy: the legs of LEGS over the cases of CASES;
  2. the log relay: the logging, epsilon-greedy and best-keeping forms, register-resident and general, append to ONE rollout log
     (random and nearest);
  3. across the episode boundary: dcm_step on an auto-resetting handle against the persistent launches, with the renewal stride set
     for the middle third of the launches, and the best log kept by the two k_bs_* forms in turn.

The schedules come from seeded generators and the oracle's episode lengths alone, so the CPU tests (not marked gpu) prove what the GPU
tests cover: every ordered pair with at least two envs in mid-episode on both sides, handovers while a task holds two waiting members,
behind the sixteenth abandonment of an agent (the overflow table), between a removal and the next join of the task."""
import numpy as np
import pytest

import helpers as H
import oracle_ref as O
import renewal_ref as R
from forms import Forms
from removal_ref import Lists, assert_handover, assert_obs, read_batch, sparse_abandoned, walk_episode

AB_CAP = 16                 # entries of an agent's abandonment log (csrc/common.hpp); further ones go to the count table
INST_SEED, CHOICE_SEED = 11, 5                  # those of test_gpu_member_removal_chunks.py: g2x3, g-ragged and rt are its walks
RAGGED_SIZES = ((70, 130), (64, 64), (65, 128), (64, 129), (70, 65), (1, 130), (20, 66), (66, 127))
LOG_CAP = 64
UNLIMITED = 1 << 40

# id: (what is set while it runs, the call).  log / best / stride: switched on or off before the launch.  obs: "all" = the three
# observation buffers, "none", "mask" = the mask alone (a partial buffer set: the general kernels at every shape).
# explore: dcm_rollout_explore over "nearest" -- with explore_q32 = 2^32 every decision is the random policy's.
LEGS = {
    "P": dict(obs="all"), "Pn": dict(obs="none"), "G": dict(obs="mask"),
    "L": dict(obs="all", log=True), "Lg": dict(obs="mask", log=True),
    "X": dict(obs="all", explore=True), "Xg": dict(obs="mask", explore=True),
    "B": dict(obs="all", log=True, best=True), "Bg": dict(obs="mask", log=True, best=True),
    "R": dict(obs="all", stride=True),
    "S": dict(step="plain"), "Sg": dict(step="leader"), "Sr": dict(step="plain", stride=True),
}
LOCKSTEP = {k for k, v in LEGS.items() if "step" in v}

# gen: the batch is made by generate_instances(INST_SEED) (the stride needs one); ranges: a ragged generated batch, loaded; sizes: per-env
# sizes on a uniform batch's arrays; req: an int = drawn from 1..that (wide).  depth: run-ins reach to that share of the second-longest
# episode; pass_pairs: at most that many handovers in a pass, so that the passes spread over the episode.  seed: of the schedule.
CASES = {
    "one": dict(A=20, T=50, B=6, mwt=2.0, gen=True, legs="P Pn G L Lg X Xg B Bg R S Sg Sr", seed=1, depth=0.6, pass_pairs=40),
    "one-ragged": dict(A=20, T=50, B=6, mwt=2.0, ranges=((10, 20), (20, 50)), legs="P Pn G L Lg X Xg B Bg S Sg", seed=2, depth=0.6, pass_pairs=40),
    "lay64": dict(A=30, T=60, B=4, mwt=2.0, legs="P Pn G L Lg X B S Sg", seed=3, depth=0.6, pass_pairs=40),
    "no-depot-lane": dict(A=10, T=64, B=4, mwt=2.0, legs="P L X B S", seed=4, depth=0.8, pass_pairs=7),
    "g2x3": dict(A=70, T=130, B=4, mwt=1.0, gen=True, legs="P Pn L X B R S Sr", seed=5, depth=0.95, pass_pairs=14),
    "g-ragged": dict(A=70, T=130, B=8, mwt=1.0, sizes=RAGGED_SIZES, legs="P L X B S", seed=6, depth=0.95, pass_pairs=5),
    "mc": dict(A=50, T=200, B=4, mwt=1.5, gen=True, legs="P Pn L X B R S", seed=17, depth=0.95, pass_pairs=11),
    "rt": dict(A=100, T=300, B=2, mwt=2.0, legs="P L X B S", seed=28, depth=0.95, pass_pairs=5),
    "wide": dict(A=24, T=9, B=8, mwt=2.0, req=16, member_cap=16, legs="P L X B S", seed=9, depth=0.95, pass_pairs=5),
}
DEEP = ("g2x3", "g-ragged", "mc", "rt", "wide")            # an agent is abandoned more than AB_CAP times in these walks
# the kernel every leg of a case must reach (the register-resident kernels carry their OBS template argument here as "+obs" / "-obs")
FAST_FORMS = {"P": "k_rollout_fast+obs", "Pn": "k_rollout_fast-obs", "G": "k_rollout_random", "L": "k_lg_rollout_fast", "Lg": "k_lg_rollout_random",
              "X": "k_ex_rollout_fast", "Xg": "k_ex_rollout_random", "B": "k_bs_rollout_fast", "Bg": "k_bs_rollout_random",
              "R": "k_rn_rollout_fast+obs", "S": "k_step_fast", "Sg": "k_step", "Sr": "k_rn_step_fast"}
GENERAL_FORMS = {"P": "k_rollout_random", "L": "k_lg_rollout_random", "X": "k_ex_rollout_random", "B": "k_bs_rollout_random", "S": "k_step"}
KERNELS = {
    "one": FAST_FORMS, "one-ragged": FAST_FORMS, "lay64": FAST_FORMS, "no-depot-lane": GENERAL_FORMS, "rt": GENERAL_FORMS, "wide": GENERAL_FORMS,
    "g2x3": dict(GENERAL_FORMS, P="k_rollout_fast_g+obs", Pn="k_rollout_fast_g-obs", R="k_rn_rollout_fast_g+obs", Sr="k_rn_step"),
    "g-ragged": dict(GENERAL_FORMS, P="k_rollout_fast_g+obs"),
    "mc": dict(GENERAL_FORMS, P="k_rollout_fast_mc+obs", Pn="k_rollout_fast_mc-obs", R="k_rn_rollout_fast_mc+obs"),
}
# 2. the log relay: the legs that write the rollout log, where the register-resident form and the general one differ
LOG_CASES = {"one": "L Lg X Xg B Bg", "lay64": "L Lg X Xg B Bg", "g2x3": "L X B"}
LOG_RUNS = [(n, p, LOG_CAP) for n in LOG_CASES for p in ("random", "nearest")] + [("one", "random", 4)]

_walks, _schedules, _lengths = {}, {}, {}


def legs_of(name):
    return CASES[name]["legs"].split()


def leg_kernel(name, leg):
    """roofline.rollout_kernel_name / step_kernel_name (pinned to csrc/plan.hpp by test_host.py) and the two form rules of plan.hpp,
    restated: the logging, epsilon-greedy and best-keeping forms exist for the one-chunk register-resident kernel and for the general
    one only (plan::form_rollout_kind), and a partial observation buffer set or a wide handle takes the general kernels
    (plan::rollout_kind).  dcm_step takes the register-resident kernel for the plain call shape on a one-chunk layout."""
    from dcmrta_amd.roofline import rollout_kernel_name, step_kernel_name
    c, leg_ = CASES[name], LEGS[leg]
    wide = c.get("member_cap", 5) > 5
    rn = "k_rn_" if leg_.get("stride") else "k_"
    if "step" in leg_:
        fast = not wide and leg_["step"] == "plain" and step_kernel_name(c["A"], c["T"]) == "k_step_fast"
        return rn + ("step_fast" if fast else "step")
    plain = "k_rollout_random" if wide or leg_["obs"] == "mask" else rollout_kernel_name(c["A"], c["T"])
    form = "k_bs_" if leg_.get("best") else "k_lg_" if leg_.get("log") else "k_ex_" if leg_.get("explore") else None
    if form:
        return form + ("rollout_fast" if plain == "k_rollout_fast" else "rollout_random")
    return rn + plain[2:] + ("" if plain == "k_rollout_random" else "+obs" if leg_["obs"] == "all" else "-obs")


def test_legs_run_the_kernels_they_name():
    """... and no two legs of a case reach the same kernel"""
    for name in CASES:
        legs = legs_of(name)
        names = {leg: leg_kernel(name, leg) for leg in legs}
        assert names == {leg: KERNELS[name][leg] for leg in legs}, (name, names)
        assert len(set(names.values())) == len(legs), (name, names)
    assert len(legs_of("one")) == len(LEGS) and len(RAGGED_SIZES) == CASES["g-ragged"]["B"]
    for name, legs in LOG_CASES.items():                     # with the log set, X / Xg are the epsilon-greedy forms still
        names = [leg_kernel(name, leg) for leg in legs.split()]
        assert len(set(names)) == len(names) and all(k[:5] in ("k_lg_", "k_ex_", "k_bs_") for k in names), (name, names)


# --------------------------------------------------------------------------------------------------------------- the oracle's side
def instances(name):
    """(instances in load_instances' keyword format, choice seeds, per-env (a, t))"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    c = CASES[name]
    B, A, T = c["B"], c["A"], c["T"]
    if c.get("gen"):                                          # what generate_instances(INST_SEED) makes on the device
        ones = [R.host_instance(A, T, INST_SEED + b, 5)[1] for b in range(B)]
        inst = {k: np.stack([i[k] for i in ones]) for k in ("depot", "task_xy", "req", "dur")}
    elif "ranges" in c:
        inst = generate_batch_ranges(range(INST_SEED, INST_SEED + B), *c["ranges"])
    else:
        inst = generate_batch(B, A, T, base_seed=INST_SEED)
        if c.get("req"):
            inst["req"] = np.random.default_rng(INST_SEED).integers(1, c["req"] + 1, (B, T)).astype(np.int32)
        if "sizes" in c:
            inst["n_agents"] = np.array([s[0] for s in c["sizes"]], np.int32)
            inst["n_tasks"] = np.array([s[1] for s in c["sizes"]], np.int32)
    sz = [(int(inst["n_agents"][b]), int(inst["n_tasks"][b])) for b in range(B)] if "n_agents" in inst else [(A, T)] * B
    return inst, env_seeds(CHOICE_SEED, 0, B), sz


def walks(oracle_lib, name):
    """(instances, seeds, sizes, per-env snapshots, the oracle's own first episode per env): computed once, read-only afterwards.  The
    walk is checked against the oracle's rollout here, every decision's record."""
    if name not in _walks:
        inst, seeds, sz = instances(name)
        mwt = CASES[name]["mwt"]
        snaps, eps = [], []
        for b, (a, t) in enumerate(sz):
            one = O.one(inst, b, t)
            s, _ = walk_episode(oracle_lib.OracleEnv(a, t, max_waiting_time=mwt).load(**one), inst["req"][b], int(seeds[b]))
            first = O.episodes(a, t, one, seeds[b], "random", 1, mwt, record=True)[0]
            assert len(s) == first["n_steps"], (name, b)
            for k in ("leader", "action", "now", "mask", "agents_obs", "tasks_obs"):
                assert np.array_equal(np.array([x[k] for x in s]).reshape(first[k].shape), first.pop(k)), (name, b, k)
            snaps.append(sparse_abandoned(s)); eps.append(first)
        _walks[name] = (inst, seeds, sz, snaps, eps)
    return _walks[name]


def lengths(oracle_lib, name, policy):
    """decisions of every env's first episode under a policy"""
    if (name, policy) not in _lengths:
        if policy == "random":
            n = [len(s) for s in walks(oracle_lib, name)[3]]
        else:
            inst, seeds, sz = instances(name)
            n = [O.episodes(a, t, O.one(inst, b, t), seeds[b], policy, 1, CASES[name]["mwt"])[0]["n_steps"] for b, (a, t) in enumerate(sz)]
        _lengths[name, policy] = np.array(n, np.int64)
    return _lengths[name, policy]


# --------------------------------------------------------------------------------------------------------------- the schedule
def closed_walk(legs, rng):
    """A closed walk over the complete directed graph of the legs that takes every edge once: k (k - 1) + 1 legs"""
    out = {u: [v for v in legs if v != u] for u in legs}
    for u in legs:
        rng.shuffle(out[u])
    stack, walk = [legs[0]], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    assert len(walk) == len(legs) * (len(legs) - 1) + 1 and walk[0] == walk[-1]
    return walk[::-1]


def build_schedule(legs, n, seed, depth, pass_pairs):
    """The launches of a relay from the episode lengths n[B] alone: (walk, passes).  A pass is a reset(), a run-in of `runin` decisions
    (P), then launches; a launch is dict(leg, amount, start, steps, pair, mid): amount = budgets int64[B] of a persistent leg (1..3,
    0 for an env whose episode is over), the number of step() calls of a lockstep leg (1..2), None = to the end of the episode;
    start / steps = decisions taken before it and by it; pair = the index in the walk of the handover in front of it when that one
    counts -- mid[B], the envs in mid-episode on both of its sides, are at least two -- else None.  A pass ends when fewer than two envs
    are left in mid-episode, after pass_pairs handovers, or with the walk; its last launch finishes the episode."""
    rng = np.random.default_rng(seed)
    walk = closed_walk(legs, rng)
    K, B = len(walk) - 1, len(n)
    reach = max(1, int(depth * np.sort(n)[-2]))

    def launch(leg, taken, last, pair, mid):
        amount = None if last else int(rng.integers(1, 3)) if leg in LOCKSTEP else np.where(taken < n, rng.integers(1, 4, B), 0).astype(np.int64)
        steps = n - taken if last else np.minimum(amount, n - taken)
        return dict(leg=leg, amount=amount, start=taken.copy(), steps=steps, pair=pair, mid=mid)

    passes, pos = [], 0
    while pos < K:
        runin = int(rng.integers(1, reach + 1))
        taken = np.minimum(runin, n)
        launches, i = [launch(walk[pos], taken, False, None, None)], pos
        while True:
            prev = launches[-1]
            taken = prev["start"] + prev["steps"]
            mid = (prev["steps"] > 0) & (taken < n)
            counts = int(mid.sum()) >= 2
            last = not counts or i + 1 == K or i + 1 - pos >= pass_pairs
            launches.append(launch(walk[i + 1], taken, last, i if counts else None, mid))
            i += counts
            if last:
                break
        assert i > pos, "a pass without a handover: choose another seed or depth"
        passes.append(dict(runin=runin, launches=launches))
        pos = i
    return walk, passes


def schedule(oracle_lib, name):
    if name not in _schedules:
        c = CASES[name]
        _schedules[name] = build_schedule(legs_of(name), lengths(oracle_lib, name, "random"), c["seed"], c["depth"], c["pass_pairs"])
    return _schedules[name]


def log_schedule(oracle_lib, name, policy):
    key = (name, policy)
    if key not in _schedules:
        _schedules[key] = build_schedule(LOG_CASES[name].split(), lengths(oracle_lib, name, policy), 100 + CASES[name]["seed"], 0.5, 40)
    return _schedules[key]


def covered_pairs(walk, passes):
    return {(walk[l["pair"]], walk[l["pair"] + 1]) for p in passes for l in p["launches"] if l["pair"] is not None}


def all_pairs(legs):
    return {(u, v) for u in legs for v in legs if u != v}


def depth_counts(name, passes, snaps, req):
    """What the handovers that count meet, from the walk: (handovers, those with a task that holds at least two members and is short of
    its requirement, those behind an agent's sixteenth abandonment, those between a removal and the next join of the task, the
    deepest decision).  An env in mid-episode on both sides of the handover must show it."""
    B = len(snaps)
    nab = [np.array([s["n_abandoned"] for s in snaps[b]]) for b in range(B)]                     # [n, t]
    join = [np.array([s["action"] - 1 for s in snaps[b]]) for b in range(B)]
    total = waiting = past = between = deepest = 0
    for p in passes:
        for l in p["launches"]:
            if l["pair"] is None:
                continue
            total += 1
            w = o = r = False
            for b in np.flatnonzero(l["mid"]):
                d = int(l["start"][b])
                s = snaps[b][d]
                deepest = max(deepest, d)
                t = len(s["members"])
                w |= any(2 <= len(m) < req[b][j] for j, m in enumerate(s["members"]))
                idx, val = s["abandoned"]
                o |= len(idx) > 0 and int(np.bincount(idx // t, val).max()) > AB_CAP
                # a removal shows between the snapshots r - 1 and r (behind decision r - 1, or in the event in front of r)
                removed = np.diff(nab[b][:d + 1], axis=0, prepend=0) != 0                    # [d + 1, t]
                for j in np.flatnonzero(removed.any(0)):
                    at = int(np.flatnonzero(removed[:, j])[-1])
                    r |= not (join[b][at:d] == j).any() and bool((join[b][d:] == j).any())
            waiting, past, between = waiting + w, past + o, between + r
    return dict(handovers=total, passes=len(passes), deepest=deepest, waiting=waiting, past_16=past, between=between)


@pytest.mark.parametrize("name", list(CASES))
def test_the_schedule_covers_every_pair_at_depth(oracle_lib, name):
    """from the walk alone, no kernel"""
    inst, _, sz, snaps, _ = walks(oracle_lib, name)
    walk, passes = schedule(oracle_lib, name)
    legs = legs_of(name)
    assert covered_pairs(walk, passes) == all_pairs(legs), name
    cnt = depth_counts(name, passes, snaps, inst["req"])
    print(name, "legs", len(legs), "pairs", len(all_pairs(legs)), cnt, "episodes", [len(s) for s in snaps])
    assert cnt["handovers"] == len(legs) * (len(legs) - 1)
    assert cnt["waiting"] >= 1 and cnt["between"] >= 1, (name, cnt)
    if name in DEEP:
        assert cnt["past_16"] >= 1, (name, cnt)
    for p in passes:                                         # an env whose episode is over: budget 0, no steps
        for l in p["launches"]:
            over = l["start"] >= lengths(oracle_lib, name, "random")
            assert (l["steps"][over] == 0).all() and (l["amount"] is None or l["leg"] in LOCKSTEP or (l["amount"][over] == 0).all())


@pytest.mark.parametrize("name,policy", [(n, p) for n in LOG_CASES for p in ("random", "nearest")])
def test_the_log_schedule_covers_every_pair(oracle_lib, name, policy):
    walk, passes = log_schedule(oracle_lib, name, policy)
    legs = LOG_CASES[name].split()
    assert covered_pairs(walk, passes) == all_pairs(legs), (name, policy)
    print(name, policy, "handovers", len(all_pairs(legs)), "passes", len(passes), "episodes", lengths(oracle_lib, name, policy).tolist())


# --------------------------------------------------------------------------------------------------------------- GPU side
def make_env(gpu_device, name, inst, **kw):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    c = CASES[name]
    env = BatchedTaskEnv(c["B"], c["A"], c["T"], device=gpu_device, max_waiting_time=c["mwt"], member_cap=c.get("member_cap", 5), **kw)
    return env.generate_instances(INST_SEED) if c.get("gen") else env.load_instances(**inst)


class Handle:
    """A handle and what is set on it: a leg switches the logs and the stride on or off before it launches."""

    def __init__(self, env, policy="random", fixed_log=None):
        self.env, self.B, self.policy, self.fixed_log = env, env.B, policy, fixed_log
        self.log = self.best = self.stride = False
        if fixed_log:                                        # 2.: set once, before reset(), and never touched
            env.enable_rollout_log(fixed_log)
            self.log = True

    def set(self, log=False, best=False, stride=False, **_):
        env = self.env
        log = log or bool(self.fixed_log)
        if self.best and not best:
            env.enable_best_log(False)
        if self.log != log:
            env.enable_rollout_log(LOG_CAP if log else 0)
        if best and not self.best:
            env.enable_best_log()
        if self.stride != stride:
            env.set_instance_renewal(self.B if stride else 0)
        self.log, self.best, self.stride = log, best, stride

    def persistent(self, leg, budget, keep=False):
        """one persistent launch of one episode under per-env budgets (keep: with the logs and the stride as they are); returns the steps"""
        import torch
        from dcmrta_amd import _lib
        from dcmrta_amd.batched_env import _ptr, check
        env, l = self.env, LEGS[leg]
        if not keep:
            self.set(**l)
        # the random policy's decisions from every form: dcm_rollout_explore with explore_q32 = 2^32 explores at every decision.
        # Under "nearest" (2.) the epsilon-greedy forms run with explore_q32 = 0
        q32 = None if not l.get("explore") else (1 << 32 if self.policy == "random" else 0)
        base = self.policy if q32 is None else "nearest"
        if l["obs"] != "mask":
            kw = {} if q32 is None else dict(explore_q32=q32)
            return env.rollout(base, episodes=1, write_obs=l["obs"] == "all", max_decisions=budget, **kw).cpu().numpy()
        steps = torch.empty((self.B,), dtype=torch.int64, device=env.device)
        per = env._dev(budget, torch.int64)
        tail = (1, -1, _ptr(per), None, None, _ptr(env._mask), _ptr(steps), env._stream())      # the mask alone
        with torch.cuda.device(env.device):
            if q32 is not None:
                check(env._lib.dcm_rollout_explore(env._h, _lib.POLICY_NEAREST, q32, *tail))
            elif base == "random":
                check(env._lib.dcm_rollout_random(env._h, *tail))
            else:
                check(env._lib.dcm_rollout_policy(env._h, env.POLICIES[base], *tail))
        return steps.cpu().numpy()

    def lockstep(self, leg, actions, keep=False):
        """one dcm_step; returns the Observation"""
        import torch
        env, l = self.env, LEGS[leg]
        if not keep:
            self.set(**l)
        if l["step"] == "plain":                             # the plain call shape: a contiguous int32 tensor on the device, nothing else
            return env.step(torch.from_numpy(actions).to(env.device))
        return env.step(actions, leader=np.full(self.B, -1, np.int32))


def _actions(mask, seeds, d, live):
    """helpers.host_random_action on the handle's own mask for the envs in mid-episode, 0 for the others"""
    act = np.zeros(len(seeds), np.int32)
    for b in np.flatnonzero(live):
        act[b] = H.host_random_action(mask[b].astype(np.uint8), int(seeds[b]), int(d[b]))
    return act


def _assert_final(env, sz, eps, tag):
    fin, sm = H.gpu_final(env), env.summary().cpu().numpy()
    for b, (a, t) in enumerate(sz):
        got = dict(fin[b])
        for k in H.FINAL_EXACT:
            got[k] = fin[b][k][:a] if k in ("travel_dist", "returned", "agent_wait") else fin[b][k][:t]
        H.assert_final_matches(got, eps[b], f"{tag} env {b}")
        O.assert_summary(sm[b], eps[b], f"{tag} env {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_state_relay(gpu_device, oracle_lib, name):
    """After every leg, for every env that ran: the steps are min(budget, decisions left); where the leg had all three buffers, the stored
    observation is the walk's record of the last decision taken; and the handle is the walk's snapshot in front of the next decision
    (assert_handover).  At the end of every pass the end state and the summary row are the oracle's."""
    c = CASES[name]
    inst, seeds, sz, snaps, eps = walks(oracle_lib, name)
    _, passes = schedule(oracle_lib, name)
    B, n, mwt = c["B"], lengths(oracle_lib, name, "random"), c["mwt"]
    lists = [Lists(t, c.get("member_cap", 5)) for _, t in sz]
    env = make_env(gpu_device, name, inst)
    h = Handle(env)

    def handover(tag, got, ran, taken):
        for b in np.flatnonzero(ran):
            assert_handover(f"{tag} env {b}: in front of decision {taken[b]}", got, b, int(taken[b]), snaps[b], lists[b], *sz[b],
                            O.one(inst, b, sz[b][1]), seeds[b], mwt)

    for ip, p in enumerate(passes):
        h.set()
        env.reset(seeds, observe=False)
        taken = np.minimum(p["runin"], n)
        assert np.array_equal(h.persistent("P", np.full(B, p["runin"], np.int64)), taken), (name, ip, "run-in")
        got = read_batch(env)
        handover(f"{name} pass {ip} run-in", got, np.ones(B, bool), taken)
        for il, l in enumerate(p["launches"]):
            leg, tag = l["leg"], f"{name} pass {ip} launch {il} ({l['leg']})"
            assert np.array_equal(taken, l["start"]), tag
            live = taken < n
            if leg in LOCKSTEP:
                obs = None
                for call in range(int((n - taken).max()) if l["amount"] is None else l["amount"]):
                    live_now = taken < n
                    obs = h.lockstep(leg, _actions(got["obs"][2] if obs is None else obs.mask.cpu().numpy(), seeds, taken, live_now))
                    taken = taken + live_now
                got = read_batch(env, obs)
                ran = live
            else:
                budget = np.where(live, UNLIMITED, 0).astype(np.int64) if l["amount"] is None else l["amount"]
                steps = h.persistent(leg, budget)
                assert np.array_equal(steps, np.minimum(budget, n - taken)), (tag, steps, budget, n - taken)
                taken = taken + steps
                ran = budget > 0
                if LEGS[leg]["obs"] == "all":                # the kernel's own stores: read before observe()
                    stored = env.obs()
                    ag, tk, mk = (x.cpu().numpy() for x in (stored.agents, stored.tasks, stored.mask))
                    for b in np.flatnonzero(ran):
                        assert_obs(f"{tag} env {b}: stored observation of decision {taken[b] - 1}", snaps[b][taken[b] - 1], *sz[b], ag[b], tk[b], mk[b])
                got = read_batch(env)
            assert np.array_equal(taken, l["start"] + l["steps"]), tag
            handover(tag, got, ran, taken)
        assert (taken == n).all(), (name, ip)
        _assert_final(env, sz, eps, f"{name} pass {ip}")
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,policy,cap", LOG_RUNS, ids=[f"{n}-{p}-cap{c}" for n, p, c in LOG_RUNS])
def test_log_relay(gpu_device, oracle_lib, name, policy, cap):
    """One rollout log, set once, appended to by the logging, epsilon-greedy and best-keeping forms in turn -- the register-held lengths
    of the k_*_rollout_fast forms against the per-step load and store of the general ones.  After every leg the log is the oracle's
    lists of the decisions taken so far: true lengths, the stored prefix, and the rows of agents beyond the env's size."""
    inst, seeds, sz = instances(name)
    _, passes = log_schedule(oracle_lib, name, policy)
    n, mwt = lengths(oracle_lib, name, policy), CASES[name]["mwt"]
    B = CASES[name]["B"]
    env = make_env(gpu_device, name, inst)
    h = Handle(env, policy=policy, fixed_log=cap)

    def check_log(tag, ran, taken):
        log = O.log(env)
        assert np.array_equal(env.status()["decisions"].cpu().numpy(), taken), tag
        for b in np.flatnonzero(ran):
            a, t = sz[b]
            o = O.play(a, t, O.one(inst, b, t), seeds[b], 0, policy, int(taken[b]), mwt)[0]
            O.assert_log(log, b, type("Played", (), dict(o=o, a=a))(), tag)

    for ip, p in enumerate(passes):
        env.reset(seeds, observe=False)
        taken = np.minimum(p["runin"], n)
        assert np.array_equal(h.persistent("L", np.full(B, p["runin"], np.int64)), taken)
        check_log(f"{name} {policy} pass {ip} run-in", np.ones(B, bool), taken)
        for il, l in enumerate(p["launches"]):
            tag = f"{name} {policy} pass {ip} launch {il} ({l['leg']})"
            budget = np.where(taken < n, UNLIMITED, 0).astype(np.int64) if l["amount"] is None else l["amount"]
            steps = h.persistent(l["leg"], budget)
            assert np.array_equal(steps, np.minimum(budget, n - taken)) and np.array_equal(steps, l["steps"]), (tag, steps, budget)
            taken = taken + steps
            check_log(tag, budget > 0, taken)
        assert (taken == n).all()
        assert (env.status()["flags"].cpu().numpy() & 1).all()
    env.close()


# --------------------------------------------------------------------------------------------------------------- 3. episode boundaries
EPISODES = 3
BOUNDARY = {"one": 3, "g2x3": 1}                            # seeds of the budgets; the CPU tests say what they must meet
S_CALLS, BUDGET_TOP = 5, 40


class Chain:
    """One env of an auto-resetting handle (auto_reset_episodes = EPISODES) in oracle episodes: dcm_step restarts it in the call that ends
    an episode until it has finished EPISODES; a persistent launch of one episode plays the episode it is in to its end, or -- if it is
    DONE and has a budget -- restarts it first.  A restart while the stride is set takes the next instance.  The decision counter
    runs on.  events: (kind of leg, launch, call in the leg, instance index) of every episode end."""

    def __init__(self, a, t, inst_of, seed, mwt):
        self.a, self.t, self.inst_of, self.seed, self.mwt = a, t, inst_of, seed, mwt
        self.idx, self.d, self.pos, self.done, self.eps, self.events, self.restarts = 0, 0, 0, False, [], [], []
        self._start(None)

    def _start(self, renew, where=None):
        if renew is not None:
            self.idx += bool(renew)
            self.restarts.append((where, bool(renew), self.idx))
        self.eps.append(O.episodes(self.a, self.t, self.inst_of(self.idx), self.seed, "random", 1, self.mwt, d0=self.d)[0])
        self.pos, self.done = 0, False

    def _advance(self, k, renew, where, restart):
        self.pos += k
        self.d += k
        if self.pos == self.eps[-1]["n_steps"]:
            self.events.append(where + (self.idx,))
            if restart and len(self.eps) < EPISODES:
                self._start(renew, where[0])
            else:
                self.done = True

    def step(self, renew, where):
        if self.done:
            return 0
        self._advance(1, renew, where, True)
        return 1

    def rollout(self, budget, renew, where):
        if budget == 0 or (self.done and len(self.eps) == EPISODES):
            return 0
        if self.done:
            self._start(renew, where[0])
        k = min(int(budget), self.eps[-1]["n_steps"] - self.pos)
        self._advance(k, renew, where, False)
        return k

    @property
    def finished(self):
        return self.done and len(self.eps) == EPISODES


def boundary_chains(name, stride):
    """The launches of the auto-reset relay and the host's model of them: S legs of S_CALLS calls and P legs of one episode under budgets
    1..BUDGET_TOP in turn, until every env has finished EPISODES episodes.  stride: set for the middle third of the launches.
    Returns (chains, launches): launches = (kind, budgets or None, stride set, steps[B] or [calls][B])."""
    c = CASES[name]
    key = ("boundary", name, stride)
    if key in _schedules:
        return _schedules[key]
    inst, seeds, sz = instances(name)
    B, mwt = c["B"], c["mwt"]

    def build(n_launches):
        rng = np.random.default_rng(BOUNDARY[name])
        chains = [Chain(*sz[b], (lambda i, b=b: R.host_instance(c["A"], c["T"], int(INST_SEED + b + i * B), 5)[1]), seeds[b], mwt) for b in range(B)]
        launches = []
        while not all(ch.finished for ch in chains):
            il = len(launches)
            on = bool(stride and n_launches and n_launches // 3 <= il < 2 * n_launches // 3)
            if il % 2 == 0:
                steps = [[ch.step(on, ("S", il, call)) for ch in chains] for call in range(S_CALLS)]
                launches.append(("S", None, on, np.array(steps, np.int64)))
            else:
                budget = np.array([0 if ch.finished else b for ch, b in zip(chains, rng.integers(1, BUDGET_TOP + 1, B))], np.int64)
                launches.append(("P", budget, on, np.array([ch.rollout(budget[b], on, ("P", il, 0)) for b, ch in enumerate(chains)], np.int64)))
            assert il < 4000
        return chains, launches

    out = build(0)
    if stride:                                               # the thirds are those of the relay without a stride: the same launches up to there
        out = build(len(out[1]))
    _schedules[key] = out
    return out


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_episode_ends_fall_on_both_sides_of_a_handover(oracle_lib, name):
    """from the oracle's episode lengths: episode ends inside both kinds of leg; a lockstep call that ends an env's episode directly in
    front of a persistent launch (on a one-chunk shape a parked final record, which that launch has to flush first), and a persistent
    launch that ends one directly in front of a lockstep call"""
    chains, launches = boundary_chains(name, False)
    ends = [e for ch in chains for e in ch.events]
    kinds = {e[0] for e in ends}
    print(name, "launches", len(launches), "episode ends in S / P legs", sum(e[0] == "S" for e in ends), sum(e[0] == "P" for e in ends),
          "episodes", [[e["n_steps"] for e in ch.eps] for ch in chains])
    assert kinds == {"S", "P"}, ends
    assert any(e[0] == "S" and e[2] == S_CALLS - 1 and e[1] + 1 < len(launches) for e in ends), ends
    assert any(e[0] == "P" and e[1] + 1 < len(launches) and launches[e[1] + 1][3].sum() > 0 for e in ends), ends
    assert all(len(ch.eps) == EPISODES for ch in chains)


def test_restarts_fall_inside_and_behind_the_stride_window(oracle_lib):
    """the stride relay on `one`: restarts that renew, in both kinds of leg, and behind the window a dcm_step restart of an env that holds
    a renewed instance -- the restart image describes instance 0 and must not come back"""
    chains, launches = boundary_chains("one", True)
    restarts = [r for ch in chains for r in ch.restarts]
    print("launches", len(launches), "restarts (leg, renewed, index)", restarts)
    assert ("S", True) in {r[:2] for r in restarts} and ("P", True) in {r[:2] for r in restarts}, restarts
    assert any(kind == "S" and not renewed and idx > 0 for kind, renewed, idx in restarts), restarts
    assert any(on for _, _, on, _ in launches) and not launches[0][2] and not launches[-1][2]


@pytest.mark.gpu
@pytest.mark.parametrize("name,stride", [("one", False), ("g2x3", False), ("one", True)], ids=["one", "g2x3", "one-stride"])
def test_auto_reset_relay(gpu_device, oracle_lib, name, stride):
    """dcm_step on an auto-resetting handle and persistent launches of one episode in turn, three episodes per env: after every leg the
    steps, the decision counters and the episode counts are the model's; at the end the return ring, summary(), the instance each env
    holds and the last episode's end state are the oracle's."""
    c = CASES[name]
    B = c["B"]
    inst, seeds, sz = instances(name)
    chains, launches = boundary_chains(name, stride)
    env = make_env(gpu_device, name, inst, auto_reset=True, auto_reset_episodes=EPISODES)
    h = Handle(env)
    ring = env.enable_return_log(4)
    obs = env.reset(seeds)
    d, eps = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for il, (kind, budget, on, steps) in enumerate(launches):
        h.set(stride=on)
        if kind == "S":
            for call in range(S_CALLS):
                active = obs.active.cpu().numpy().astype(bool)
                assert np.array_equal(active, steps[call] > 0), (name, il, call, active, steps[call])
                obs = h.lockstep("S", _actions(obs.mask.cpu().numpy(), seeds, d, active), keep=True)
                d += steps[call]
        else:
            got = h.persistent("P", budget, keep=True)
            assert np.array_equal(got, steps), (name, il, got, steps, budget)
            d += steps
            obs = env.observe()
        for b, ch in enumerate(chains):
            eps[b] = sum(1 for e in ch.events if e[1] <= il)
        assert np.array_equal(env.status()["decisions"].cpu().numpy(), d), (name, il)
        assert np.array_equal(env.episodes().cpu().numpy(), eps), (name, il, eps)
    assert not obs.active.cpu().numpy().any()
    rl, sm, hd = ring.cpu().numpy(), env.summary().cpu().numpy(), R.held(env)
    idx = env.instance_index().cpu().numpy() if c.get("gen") else np.zeros(B, np.int64)
    fin = H.gpu_final(env)
    for b, ch in enumerate(chains):
        assert d[b] == sum(e["n_steps"] for e in ch.eps) and eps[b] == EPISODES
        assert [rl[b, k] for k in range(EPISODES)] == [e["reward"] for e in ch.eps], (name, b)
        assert np.isnan(rl[b, EPISODES]), (name, b)
        O.assert_summary(sm[b], ch.eps[-1], (name, b))
        assert idx[b] == ch.idx, (name, b, idx[b], ch.idx)
        R.assert_instance(hd, b, (sz[b][0], ch.inst_of(ch.idx)))
        H.assert_final_matches(fin[b], ch.eps[-1], f"{name} env {b}")
    if stride:
        assert {ch.idx for ch in chains} != {0}
    env.close()


# the shape of `one` as a forms.py entry: uniform_base + 3 A + T = INST_SEED, so its instances and seeds are those of `one`
BEST = Forms({"one": (20, 50, 6, dict(max_waiting_time=2.0), None, -1)}, {}, INST_SEED - 3 * 20 - 50, 0, CHOICE_SEED)


@pytest.mark.gpu
def test_best_log_across_families(gpu_device, oracle_lib):
    """Three episodes per env as k_bs_rollout_fast and k_bs_rollout_random launches in turn under budgets 1..40: the kept episode, its
    summary row and its routes are what the order of include/dcmrta_env.h keeps of the oracle's three episodes."""
    env, seeds = BEST.env(gpu_device, "one")
    B, inst = env.B, BEST.instances("one")[0]
    orc = BEST.episodes("one", "random", EPISODES)
    n = np.array([[r["n_steps"] for r in O.episodes(20, 50, O.one(inst, b), seeds[b], "random", EPISODES, 2.0)] for b in range(B)], np.int64)
    h = Handle(env)
    h.set(log=True, best=True)
    env.reset(seeds, observe=False)
    rng = np.random.default_rng(17)
    left = n.sum(1)
    ends = np.cumsum(n, 1)
    taken = np.zeros(B, np.int64)
    for il in range(4000):
        if not left.any():
            break
        budget = np.where(left > 0, rng.integers(1, BUDGET_TOP + 1, B), 0).astype(np.int64)
        # one episode per launch: an env stops at the end of the episode it is in
        want = np.array([min(budget[b], int(ends[b][np.searchsorted(ends[b], taken[b], side="right")] - taken[b])) if left[b] else 0 for b in range(B)])
        steps = h.persistent("B" if il % 2 == 0 else "Bg", budget, keep=True)
        assert np.array_equal(steps, want), (il, steps, want, budget)
        taken, left = taken + steps, left - steps
    assert not left.any()
    task, arrival, length = (x.cpu().numpy() for x in env.best_routes())
    kept, sm = env.best_episode().cpu().numpy(), env.best_summary().cpu().numpy()
    for b in range(B):
        fin = [e.o.final() for e in orc[b]]
        order = [(int(f["finished"].sum()), f["reward"]) for f in fin]
        assert int(kept[b]) == max(range(EPISODES), key=lambda i: (order[i], -i)), (b, order, kept[b])          # the earliest of the best
        assert (sm[b, 1], sm[b, 0]) == order[int(kept[b])], b
        O.assert_log((task, arrival, length), b, orc[b][int(kept[b])], f"best env {b}")
    assert np.array_equal(env.episodes().cpu().numpy(), np.full(B, EPISODES))
    env.close()
