"""-m gpu: every kernel family away from the reference's max_waiting_time 10 / max_time 100 and on degenerate instances.

The table (param_edges_ref.FORMS; it is shared with test_param_edges_host.py, which proves on the CPU what the cases reach) holds the
smallest shape that selects each kernel -- one chunk at runtime and compile-time sizes, Lay{64,64}, the mid sizes in every chunk
count, 50A/200T, a wide handle -- under four (max_waiting_time, max_time) sets: 10 / 30 (the limit cuts episodes with work left),
3 / 250 (hundreds of abandonments: the 16-entry log overflows into the count table), 25 / 100 and 1e6 / 100 (nobody is abandoned for
waiting; an env whose agents all wait ends when its clock jumps to arrival + 1e6).  Five shapes also play forms.degenerate instances
at 10 / 100 (coincident tasks, tasks on the depot, durations 0), and two a budgeted row at max_waiting_time 1e-9, the smallest
positive waiting time, which keeps the register-resident kernels (200 decisions under each of the three policies: the oracle plays
them all, no policy is left out).

Yardstick: the oracle, threaded through the shared reference layer with max_time.  Every comparison is exact; there is no tolerance."""
import numpy as np
import pytest

import helpers as H
import lookahead_policy_ref as LP
import lookahead_ref as LA
import oracle_ref as O
import param_edges_ref as PE
import removal_ref as RR
import renewal_ref as R
from forms import assert_same, snap

pytestmark = pytest.mark.gpu

FORMS, F = PE.FORMS, PE.F                       # base seeds: PE.UNIFORM_BASE, PE.RAGGED_BASE, PE.CHOICE_BASE
CAP = 32                                        # entries per agent of the rollout log: at 3 / 250 a route outgrows it, its prefix is kept
CUT, MANY = "w10-t30", "w3-t250"
OBS_KEYS = ("agents", "tasks", "mask")
LOG_KEYS = ("log_task", "log_arrival", "log_len")


def ids(shapes, params):
    return [PE.form_id(s, p) for s in shapes for p in params] + [PE.form_id(s, "degenerate") for s in shapes if s in PE.DEGENERATE_SHAPES]


def _env(gpu_device, form, ring=3, log=0, best=False):
    env, seeds = F.env(gpu_device, form)
    if log:
        env.enable_rollout_log(log)
    if best:
        env.enable_best_log()
    env._ring = env.enable_return_log(ring)
    env.reset(seeds, observe=False)
    return env, seeds


def _without(s, keys):
    return {k: v for k, v in s.items() if k not in keys}


def _sorted_log_rows(s, env):
    """A snapshot of a uniform handle with every agent's abandonment-log row sorted.  The state blob ends with the side tables
    (csrc/common.hpp side_bytes): u16[B][A][16] log rows, then the count tables of align16(2 A T) bytes per env."""
    B, A, T = env.B, env.A, env.T
    rows, side = B * A * 16 * 2, B * A * 16 * 2 + B * ((2 * A * T + 15) & ~15)
    state = s["state"].copy()
    assert state.dtype == np.uint8 and state.ndim == 1 and state.size == B * env.record_bytes() + B * 64 + side
    state[state.size - side:state.size - side + rows].view(np.uint16).reshape(B * A, 16).sort(axis=1)
    return dict(s, state=state)


def _cut(fin, a, t):
    """H.gpu_final's dict of one env at the env's own sizes"""
    return {k: (v[:a] if k in ("travel_dist", "returned", "agent_wait") else v[:t] if k in H.FINAL_EXACT else v) for k, v in fin.items()}


def _assert_episode(env, b, a, t, ref, tag, fin=None, sm=None):
    """env b after a whole episode against the oracle's terminal results `ref`: every per-task and per-agent quantity, the six metrics,
    the reward, the summary row and the header flags"""
    fin = H.gpu_final(env) if fin is None else fin
    sm = env.summary().cpu().numpy() if sm is None else sm
    H.assert_final_matches(_cut(fin[b], a, t), ref, tag)
    O.assert_summary(sm[b], ref, tag)
    assert fin[b]["flags"] == PE.expected_flags(ref), (tag, "flags", fin[b]["flags"], PE.expected_flags(ref))


def _assert_stopped(env, b, a, t, o, d, tag, fin, st):
    """env b where a budget stopped it, against the OracleEnv the same cap stopped: what is defined in mid-episode"""
    ref = o.final()
    assert st["decisions"][b] == d and st["now"][b] == o.now and not st["flags"][b] & 1, (tag, int(st["decisions"][b]), d, st["now"][b], o.now)
    f = _cut(fin[b], a, t)
    for k in ("finished", "feasible", "time_start", "time_finish", "n_members", "n_abandoned", "travel_dist", "returned"):
        assert np.array_equal(np.asarray(f[k]).astype(ref[k].dtype), ref[k]), (tag, k)


# ---------------------------------------------------------------------------------------------------- 1. three episodes in one launch
@pytest.mark.parametrize("policy", PE.POLICIES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_three_episodes_against_the_oracle(gpu_device, form, policy):
    """rollout(policy, episodes=3) with all observation buffers and with none (the two template arguments of the register-resident
    kernels): steps against Sim.launch, the three returns (the first two come from the metric-free terminal), every terminal quantity
    of the third episode, its summary row and flags; and the two launches leave the same bytes.  A tiny row stops at its budget in
    mid-episode and is compared with the oracle stopped by the same cap."""
    PE.check_case(form, policy)
    budget = FORMS[form][5]
    sims, ref_steps = F.sims(form, policy, 3)
    returns = None if budget >= 0 else [[e.o.final()["reward"] for e in eps] for eps in F.episodes(form, policy, 3)]
    snaps = {}
    for obs in (True, False):
        tag = f"{form} {policy} {'obs' if obs else 'no obs'}"
        env, _ = _env(gpu_device, form)
        steps = env.rollout(policy, episodes=3, write_obs=obs, max_decisions=budget).cpu().numpy()
        assert np.array_equal(steps, ref_steps), (tag, steps, ref_steps)
        fin, sm, ring = H.gpu_final(env), env.summary().cpu().numpy(), env._ring.cpu().numpy()
        st, eps_done = {k: v.cpu().numpy() for k, v in env.status().items()}, env.episodes().cpu().numpy()
        for b, ((a, t), s) in enumerate(zip(PE.sizes(form), sims)):
            if budget >= 0:
                assert not s.done
                _assert_stopped(env, b, a, t, s.o, int(ref_steps[b]), f"{tag} env{b}", fin, st)
                assert np.isnan(ring[b, s.j:]).all() and not np.isnan(ring[b, :s.j]).any() and eps_done[b] == s.j, (tag, b, ring[b], s.j)
                assert s.j or np.isnan(sm[b]).all(), (tag, b)
            else:
                assert s.done and st["decisions"][b] == ref_steps[b], (tag, b)      # the counter runs on across the episodes
                assert np.array_equal(ring[b], np.array(returns[b])), (tag, b, ring[b], returns[b])
                _assert_episode(env, b, a, t, s.o.final(), f"{tag} env{b}", fin, sm)
        snaps[obs] = snap(env, steps)
        env.close()
    assert_same(_without(snaps[False], OBS_KEYS), _without(snaps[True], OBS_KEYS), f"{form} {policy}: with and without observation buffers")


# ---------------------------------------------------------------------------------------------------- 2. the mask buffer alone
@pytest.mark.parametrize("policy", PE.POLICIES)
@pytest.mark.parametrize("form", ids(("small", "exact", "mc"), PE.PARAMS) + [PE.form_id(s, "tiny") for s in PE.TINY_SHAPES])
def test_a_partial_buffer_set_plays_the_general_kernel_to_the_same_bytes(gpu_device, form, policy):
    """The general kernel at the one-chunk shapes and at 50A/200T against the register-resident kernels: every byte a launch leaves.
    One exception, decided by the oracle alone: where its walk of the same launch shows an agent dropped by two tasks in ONE
    task_update pass (param_edges_ref.double_drops; small-tiny under random: agent 1 of env 0, tasks 4 and 11), the abandonment-log
    rows are compared as multisets.  The order of the entries of one pass is not part of the state -- the general kernel takes it
    from the order in which its lanes' atomics land, and every reader sorts the row (compute_waits) or only counts it."""
    budget = FORMS[form][5]
    full, _ = _env(gpu_device, form)
    ref = snap(full, full.rollout(policy, episodes=3, max_decisions=budget).cpu().numpy())
    env, _ = _env(gpu_device, form)
    got = snap(env, H.rollout_mask_only(env, policy, 3, budget))
    assert np.array_equal(got["steps"], F.sims(form, policy, 3)[1]), (form, policy)
    got, ref = (_without(s, ("agents", "tasks")) for s in (got, ref))
    if got["state"].tobytes() != ref["state"].tobytes() and any(PE.double_drops(form, policy)):     # (the walk is made only where it decides)
        got, ref = _sorted_log_rows(got, env), _sorted_log_rows(ref, env)
    assert_same(got, ref, f"{form} {policy}: the mask alone")


# ---------------------------------------------------------------------------------------------------- 3. a budget stop and a handover
@pytest.mark.parametrize("form", ids(("small", "no-depot-lane", "mc", "wide"), (CUT, MANY)))
def test_a_budget_stop_hands_the_episode_over(gpu_device, form):
    """Random policy, every env stopped after a third of its own first episode (per-env budgets): the handle against the oracle walk's
    snapshot in front of the pending decision (removal_ref.assert_handover: member lists, abandonment counts, task and agent side,
    the observation).  Then an unlimited launch of three episodes against Sim."""
    mwt, mt = PE.params_of(form)
    inst, seeds = F.instances(form)
    sz, n = PE.sizes(form), PE.first_lengths(form, "random")
    at = np.array([max(1, k // 3) for k in n], np.int64)
    snaps = PE.handover_walks(form)
    assert [len(s) for s in snaps] == n, form
    env, _ = _env(gpu_device, form)
    assert np.array_equal(env.rollout("random", episodes=1, max_decisions=at).cpu().numpy(), at)
    got = RR.read_batch(env)
    sims = []
    for b, (a, t) in enumerate(sz):
        one = O.one(inst, b, t)
        RR.assert_handover(f"{form} env {b}: in front of decision {at[b]}", got, b, int(at[b]), snaps[b], RR.Lists(t, env.member_cap), a, t,
                           one, seeds[b], mwt, mt)
        sims.append(O.Sim(a, t, lambda j, one=one: one, seeds[b], "random", mwt, mt))
        assert sims[b].launch(1, int(at[b])) == at[b] and not sims[b].done
    steps = env.rollout("random", episodes=3).cpu().numpy()
    ref_steps = np.array([s.launch(3, -1) for s in sims], np.int64)
    assert np.array_equal(steps, ref_steps), (form, steps, ref_steps)
    fin, sm = H.gpu_final(env), env.summary().cpu().numpy()
    for b, (a, t) in enumerate(sz):
        _assert_episode(env, b, a, t, sims[b].o.final(), f"{form} env{b} behind the handover", fin, sm)
    assert (env.episodes().cpu().numpy() == 3).all()


# ---------------------------------------------------------------------------------------------------- 4. the rollout log
@pytest.mark.parametrize("policy", ["nearest", "random"])
@pytest.mark.parametrize("form", ids(("small", "mid", "mc", "wide"), (CUT, MANY)))
def test_the_logging_forms_log_the_oracles_routes(gpu_device, form, policy):
    """enable_rollout_log: the third episode's routes and arrival times are the oracle's lists (an episode that stops at max_time ends
    in mid-route; at 3 / 250 a route is longer than the log's cap and its prefix is kept), everything else is the unlogged launch's."""
    plain, _ = _env(gpu_device, form)
    ref = snap(plain, plain.rollout(policy, episodes=3).cpu().numpy())
    env, _ = _env(gpu_device, form, log=CAP)
    got = snap(env, env.rollout(policy, episodes=3).cpu().numpy())
    assert_same(_without(got, LOG_KEYS), ref, f"{form} {policy}: the logged launch")
    sims, ref_steps = F.sims(form, policy, 3)
    assert np.array_equal(got["steps"], ref_steps)
    log = O.log(env)
    for b, s in enumerate(sims):
        O.assert_log(log, b, s, f"{form} {policy}")
    if form == PE.form_id("mc", MANY) and policy == "random":
        assert max(len(s.o.route(a)[0]) for s in sims for a in range(s.a)) > CAP, (form, "no route of the oracle's outgrows the log")


# ---------------------------------------------------------------------------------------------------- 5. epsilon-greedy
EXPLORE_FORMS = ids(("small", "no-depot-lane", "mc"), (CUT, MANY))


@pytest.mark.parametrize("form", EXPLORE_FORMS)
def test_the_ends_of_explore_are_nearest_and_random(gpu_device, form):
    for q32, pinned in ((0, "nearest"), (1 << 32, "random")):
        twin, _ = _env(gpu_device, form)
        ref = snap(twin, twin.rollout(pinned, episodes=3).cpu().numpy())
        env, _ = _env(gpu_device, form)
        got = snap(env, env.rollout("nearest", episodes=3, explore_q32=q32).cpu().numpy())
        assert_same(got, ref, f"{form} q={q32}")
        assert np.array_equal(got["steps"], F.sims(form, pinned, 3)[1]), (form, q32)


def _assert_explore_episodes(env, steps, form, cases, tag):
    """three episodes at epsilon 0.25 against the oracle walk: steps, returns, the third episode's results, flags and logged routes"""
    fin, sm, ring, log = H.gpu_final(env), env.summary().cpu().numpy(), env._ring.cpu().numpy(), O.log(env)
    for b, ((a, t), eps) in enumerate(zip(PE.sizes(form), cases)):
        assert steps[b] == sum(e["n_steps"] for e in eps), (tag, b, steps[b], [e["n_steps"] for e in eps])
        assert np.array_equal(ring[b], np.array([e["result"]["reward"] for e in eps])), (tag, b)
        _assert_episode(env, b, a, t, eps[-1]["result"], f"{tag} env{b}", fin, sm)
        O.assert_log(log, b, LP.Episode(eps[-1]), tag)


@pytest.mark.parametrize("form", EXPLORE_FORMS)
def test_explore_at_a_quarter_against_the_oracle_walk(gpu_device, form):
    cases = PE.explore_cases(form)
    assert any(0 < e["explored"] < e["n_steps"] for eps in cases for e in eps), form         # both branches were taken
    env, _ = _env(gpu_device, form, log=CAP)
    steps = env.rollout("nearest", episodes=3, explore=0.25).cpu().numpy()
    _assert_explore_episodes(env, steps, form, cases, f"{form} epsilon 0.25")


# ---------------------------------------------------------------------------------------------------- 6. the best log and its reduction
@pytest.mark.parametrize("form", [PE.form_id("small", CUT), PE.form_id("mid", CUT), PE.form_id("small", "degenerate")])
def test_the_best_log_keeps_the_best_of_three_cut_episodes(gpu_device, form):
    """Three episodes at epsilon 0.25 under max_time 30 with the best log on: the kept episode per env is the best of the oracle's three
    under the strict (finished tasks, reward) order -- candidates end with unfinished tasks here, so the first key decides, which it
    never does at 10 / 100 -- and reduce_best(group=2) gives what a sequential scan of each pair of envs gives."""
    T, B = FORMS[form][1], FORMS[form][2]
    cases = PE.explore_cases(form)
    pairs = [[LA.pair(e["result"]) for e in eps] for eps in cases]
    assert any(len({p[0] for p in ps}) > 1 for ps in pairs), (form, pairs)                 # the first key decides in some env
    if PE.split(form)[1] == CUT:
        assert any(p[0] < T for ps in pairs for p in ps), (form, pairs)
    if form == PE.form_id("small", CUT):
        assert all(p[0] < T for ps in pairs for p in ps), pairs
    env, _ = _env(gpu_device, form, log=CAP, best=True)
    steps = env.rollout("nearest", episodes=3, explore=0.25).cpu().numpy()
    _assert_explore_episodes(env, steps, form, cases, f"{form} best")
    best = tuple(x.cpu().numpy() for x in env.best_routes())
    bsm, bep = env.best_summary().cpu().numpy(), env.best_episode().cpu().numpy()
    keep = [PE.kept(eps) for eps in cases]
    for b, eps in enumerate(cases):
        assert bep[b] == keep[b], (form, b, int(bep[b]), keep[b], pairs[b])
        assert bsm[b].tobytes() == O.summary_row(eps[keep[b]]["result"]).tobytes(), (form, b)
        O.assert_log(best, b, LP.Episode(eps[keep[b]]), f"{form} best routes")
    red = {k: v.cpu().numpy() for k, v in env.reduce_best(group=2).items()}
    for g in range(B // 2):
        w = 2 * g
        if pairs[2 * g + 1][keep[2 * g + 1]] > pairs[w][keep[w]]:                            # strict: a tie stays with the lower env
            w = 2 * g + 1
        assert red["env"][g] == w and red["episode"][g] == keep[w] and red["summary"][g].tobytes() == bsm[w].tobytes(), (form, g)
        assert np.array_equal(red["len"][g], best[2][w]), (form, g)
        inside = np.arange(CAP)[None, :] < np.minimum(best[2][w], CAP)[:, None]
        assert np.array_equal(red["task"][g], np.where(inside, best[0][w], -2)), (form, g)
        assert red["arrival"][g].tobytes() == np.where(inside, best[1][w], 0.0).tobytes(), (form, g)


# ---------------------------------------------------------------------------------------------------- 7. lookahead
@pytest.mark.parametrize("width", [None, 2], ids=["all", "width2"])
@pytest.mark.parametrize("form", ids(("small", "few-agents"), (CUT, MANY)))
def test_lookahead_against_the_oracle_walker(gpu_device, form, width):
    """rollout("nearest", lookahead=True) and width=2, return_inner=True.  At 10 / 30 every inner episode ends at max_time, values tie
    on -now and the lowest action index decides; on the degenerate instances distances tie as well.  At 3 / 250 `nearest` plays the
    first half of its episode, the lookahead rule two decisions -- its inner episodes run through hundreds of abandonments and the
    snapshot they restore holds a filled abandonment log -- and `nearest` the rest."""
    cases = PE.lookahead_cases(form, width)
    kw = dict(lookahead=True) if width is None else dict(lookahead=True, width=width, return_inner=True)
    env, _ = _env(gpu_device, form, log=CAP)
    B = env.B
    if cases[0]["whole"]:
        out = env.rollout("nearest", episodes=1, write_obs=False, **kw)
        walks, inner = [c["w"] for c in cases], [c["w"].get("inner") for c in cases]
    else:
        d0 = np.array([c["d0"] for c in cases], np.int64)
        assert np.array_equal(env.rollout("nearest", episodes=1, max_decisions=d0).cpu().numpy(), d0)
        out = env.rollout("nearest", episodes=1, write_obs=False, max_decisions=PE.LOOKAHEAD_WINDOW_K, **kw)
        walks, inner = [c["tail"] for c in cases], [c["window"].get("inner") for c in cases]
        assert all(c["window"]["n_steps"] == c["d0"] + PE.LOOKAHEAD_WINDOW_K and not c["window"]["ended"] for c in cases)
        assert any(f["n_unmasked"] > 2 for c in cases for f in c["window"]["facts"]), form
    steps = (out if width is None else out[0]).cpu().numpy()
    if width is not None:
        assert np.array_equal(out[1].cpu().numpy(), np.array(inner, np.int64)), (form, out[1].cpu().numpy(), inner)
    if not cases[0]["whole"]:
        assert (steps == PE.LOOKAHEAD_WINDOW_K).all()
        steps = d0 + steps + env.rollout("nearest", episodes=1).cpu().numpy()
    fin, sm = H.gpu_final(env), env.summary().cpu().numpy()
    st, log = env.status()["decisions"].cpu().numpy(), O.log(env)
    for b, ((a, t), w) in enumerate(zip(PE.sizes(form), walks)):
        tag = f"{form} lookahead {width} env{b}"
        assert steps[b] == w["n_steps"] == st[b], (tag, steps[b], w["n_steps"], st[b])
        _assert_episode(env, b, a, t, w["result"], tag, fin, sm)
        assert fin[b]["flags"] == w["flags"], tag
        O.assert_log(log, b, LP.Episode(w), tag)
    assert (env.episodes().cpu().numpy() == 1).all() and B == len(cases)


# ---------------------------------------------------------------------------------------------------- 8. instance renewal
RENEWAL_BASE = 9300


@pytest.mark.parametrize("policy", ["random", "nearest"])
@pytest.mark.parametrize("form", [PE.form_id(s, p) for s in ("small", "mid", "mc") for p in (CUT, MANY)])
def test_three_episodes_under_instance_renewal(gpu_device, form, policy):
    """generate_instances + set_instance_renewal(B): episode k of env b plays instance RENEWAL_BASE + k B + b, and the abandonment
    tables of episode k - 1 are gone (the k_rn_* forms of every layout)."""
    A, T, B, kw, _, _ = FORMS[form]
    mwt, mt = PE.params_of(form)
    from dcmrta_amd.choice import env_seeds
    seeds = env_seeds(PE.CHOICE_BASE + 1, 0, B)
    chains = {b: R.oracle_chain(A, T, RENEWAL_BASE + b, B, int(seeds[b]), policy=policy, mwt=mwt, max_time=mt) for b in range(B)}
    rows = np.array([e["row"] for b in range(B) for e in chains[b][0]])
    if PE.split(form)[1] == CUT and (PE.split(form)[0] != "mid" or policy == "random"):    # (`nearest` finishes 66A/70T inside 30)
        assert (rows[:, 1] < T).any(), form                                               # episodes the limit cut
    for obs in (True, False):
        env, ring = R.make(gpu_device, B, A, T, RENEWAL_BASE, B, **kw)
        env.reset(seeds, observe=False)
        steps = env.rollout(policy, episodes=3, write_obs=obs).cpu().numpy()
        R.assert_after(env, ring, chains, steps)
        env.close()


# ---------------------------------------------------------------------------------------------------- 9. lockstep
@pytest.mark.parametrize("form", ids(("chunks", "mc", "wide"), (CUT, MANY)))
def test_lockstep_against_the_recorded_oracle_rollout(gpu_device, form):
    """dcm_step with the host random policy: leader, event time, mask and both observation tensors of every decision, then the
    terminal results."""
    mwt, mt = PE.params_of(form)
    inst, seeds = F.instances(form)
    env, _ = F.env(gpu_device, form)
    got = H.run_lockstep(env, seeds, lambda b, i, mask, l: H.host_random_action(mask, int(seeds[b]), i))
    fin, sm = H.gpu_final(env), env.summary().cpu().numpy()
    for b, (a, t) in enumerate(PE.sizes(form)):
        ref = O.episodes(a, t, O.one(inst, b, t), seeds[b], "random", 1, mwt, record=True, max_time=mt)[0]
        assert got[b]["n_steps"] == ref["n_steps"], (form, b, got[b]["n_steps"], ref["n_steps"])
        for k in ("leader", "action", "now", "mask", "agents_obs", "tasks_obs"):
            assert got[b][k].tobytes() == np.ascontiguousarray(ref[k]).astype(got[b][k].dtype).tobytes(), (form, b, k)
        _assert_episode(env, b, a, t, ref, f"{form} lockstep env{b}", fin, sm)


def test_auto_reset_parks_the_terminal_of_an_unfinished_episode(gpu_device):
    """auto_reset at 10 / 30 through two episode ends: both episodes stop at max_time with work left, their final records are parked
    and flushed later (k_step_fast, k_terminal_flush); returns and the last summary row against the oracle."""
    form = PE.form_id("small", CUT)
    A, T, B, kw, _, _ = FORMS[form]
    mwt, mt = PE.params_of(form)
    inst, seeds = F.instances(form)
    assert all(e["ending"] == "max-time" for env in PE.facts(form, "random") for e in env[:2])
    env = H.sized_env(gpu_device, A, T, inst, auto_reset=True, auto_reset_episodes=2, **kw)
    ring = env.enable_return_log(2)
    taken = R.lockstep_to_end(env, seeds)
    sm, ring = env.summary().cpu().numpy(), ring.cpu().numpy()
    for b in range(B):
        eps = O.episodes(A, T, O.one(inst, b), seeds[b], "random", 2, mwt, max_time=mt)
        assert taken[b] == sum(e["n_steps"] for e in eps), (b, taken[b])
        assert np.array_equal(ring[b], np.array([e["reward"] for e in eps])), (b, ring[b])
        O.assert_summary(sm[b], eps[-1], f"auto-reset env{b}")
    assert (env.episodes().cpu().numpy() == 2).all()


# ---------------------------------------------------------------------------------------------------- 10. fork
@pytest.mark.parametrize("form", ids(("mc", "wide"), (MANY,)))
def test_a_fork_in_mid_episode_carries_the_abandonment_tables(gpu_device, form):
    """fork_from three quarters into the first random episode: the abandonment log is filled (and on 50A/200T overflowed into the
    count table, on a multi-chunk layout); the copy played on equals the source played on, and both equal the oracle."""
    at, most = PE.fork_points(form)
    assert max(most) > (PE.AB_CAP if form == PE.form_id("mc", MANY) else 0), (form, most)
    src, _ = _env(gpu_device, form)
    at = np.array(at, np.int64)
    assert np.array_equal(src.rollout("random", episodes=1, max_decisions=at).cpu().numpy(), at)
    dst, _ = _env(gpu_device, form)
    dst.fork_from(src, np.arange(src.B, dtype=np.int32), check=True)
    assert np.array_equal(dst.abandoned_counts().cpu().numpy(), src.abandoned_counts().cpu().numpy())
    ref = snap(src, src.rollout("random", episodes=2).cpu().numpy())
    got = snap(dst, dst.rollout("random", episodes=2).cpu().numpy())
    assert_same(got, ref, f"{form}: the fork played on")
    sims, ref_steps = F.sims(form, "random", 2)
    assert np.array_equal(at + got["steps"], ref_steps), form
    fin, sm = H.gpu_final(dst), dst.summary().cpu().numpy()
    for b, (a, t) in enumerate(PE.sizes(form)):
        _assert_episode(dst, b, a, t, sims[b].o.final(), f"{form} fork env{b}", fin, sm)
