"""-m gpu: the greedy device policies of the persistent rollout (dcm_rollout_policy: DCM_POLICY_FIRST, DCM_POLICY_NEAREST) on the
register-resident form (k_hp_rollout_fast) and the general form (k_hp_rollout_random), plain and renewing.

Yardsticks: the reference-generated golden traces under `first` / `nearest`, and beyond them the oracle's policy_pick
(oracle/dcmrta_oracle.c).  Every comparison is bit for bit: observation tensors as fp32 bit patterns, masks, summary rows, returns,
step counts, task and agent getters."""
import functools
import glob
import os

import numpy as np
import pytest

import helpers as H
import oracle_ref as O

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
POLICIES = ("first", "nearest")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _obs(env):
    o = env.obs()
    return tuple(x.clone().cpu().numpy() for x in (o.agents, o.tasks, o.mask))


def _assert_stored(got, ref, b, k, a, t, tag):
    """What the kernel stored for the last decision taken by env b (decision k of ref), rows of the env's own sizes (a, t)."""
    ag, tk, mk = got
    assert np.array_equal(_bits(ag[b, :a]), _bits(ref["agents_obs"][k])), f"{tag} env{b} decision {k}: agents observation"
    assert np.array_equal(_bits(tk[b, :t + 1]), _bits(ref["tasks_obs"][k])), f"{tag} env{b} decision {k}: tasks observation"
    assert np.array_equal(mk[b, :t + 1].astype(np.uint8), ref["mask"][k]), f"{tag} env{b} decision {k}: mask"


# ---------------------------------------------------------------------------------------------------- 1. reference goldens
def _golden_groups():
    g = {}
    for pol in POLICIES:
        for p in sorted(glob.glob(os.path.join(H.GOLDEN, f"trace_*_{pol}_s*.npz"))):
            tr = H.load_trace(p)
            g.setdefault((int(tr["A"]), int(tr["T"]), pol), []).append((os.path.basename(p), tr))
    return g


def _removal_decisions(tr):
    """Decisions whose observation shows a task with MORE open slots than the decision before saw: members were removed in between."""
    st = tr["tasks_obs"][:, 1:, 0]
    return np.flatnonzero((st[1:] > st[:-1]).any(axis=1)) + 1


def _stops(tr):
    """Five decision indices to stop after: the first, the last, three in between -- one of them the decision right after a member
    removal wherever the trace holds one."""
    n = int(tr["n_steps"])
    mid = [n // 4, n // 2, (3 * n) // 4]
    rem = [k for k in _removal_decisions(tr) if 0 < k < n - 1]
    if rem:
        mid[1] = int(rem[len(rem) // 2])
    return sorted(set([0, n - 1] + mid))


# the full traces in which no member is ever removed (every `first` trace, two `nearest` ones): they get three evenly spaced stops
NO_REMOVAL = {"trace_5A8T_first_s0.npz", "trace_5A8T_first_s1.npz", "trace_10A20T_first_s0.npz", "trace_10A20T_first_s1.npz",
              "trace_20A50T_first_s0.npz", "trace_20A50T_first_s1.npz", "trace_10A20T_nearest_s1.npz", "trace_20A50T_nearest_s1.npz"}


def test_golden_set_holds_what_the_stops_need():
    g = _golden_groups()
    assert sorted(g) == [(5, 8, "first"), (5, 8, "nearest"), (10, 20, "first"), (10, 20, "nearest"), (20, 50, "first"), (20, 50, "nearest"),
                         (50, 200, "nearest")]
    assert sum(len(v) for v in g.values()) == 13
    for v in g.values():
        for name, tr in v:
            stops, rem = _stops(tr), _removal_decisions(tr)
            assert stops[0] == 0 and stops[-1] == int(tr["n_steps"]) - 1 and len(stops) == 5, name
            # every trace that holds a removal is stopped right after one; the others are exactly the listed ones
            assert (len(rem) == 0) == (name in NO_REMOVAL), (name, rem)
            assert name in NO_REMOVAL or any(k in rem for k in stops[1:-1]), (name, stops, rem)
    with_removal = {name.split("_")[1] for v in g.values() for name, _ in v if name not in NO_REMOVAL}
    assert with_removal == {"5A8T", "10A20T", "20A50T", "50A200T"}                          # every shape has such a stop


@pytest.mark.parametrize("A,T,policy", sorted(_golden_groups()))
def test_reference_goldens_through_the_persistent_kernel(gpu_device, A, T, policy):
    """Every full `first` / `nearest` trace the reference generated, played by dcm_rollout_policy (5A/8T, 10A/20T, 20A/50T: the
    register-resident form; 50A/200T: the general one), stopped by budget at five decisions per trace: the kernel's own stores of that
    decision, then the terminal results."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    traces = _golden_groups()[(A, T, policy)]
    B = len(traces)
    env = BatchedTaskEnv(B, A, T, device=gpu_device)
    env.load_instances(*[np.stack([t[k] for _, t in traces]) for k in ("depot", "task_xy", "req", "dur")])
    env.reset(np.array([int(t["seed_e"]) for _, t in traces], np.uint64), observe=False)
    stops = [_stops(t) for _, t in traces]
    taken = np.zeros(B, np.int64)
    for s in range(max(len(x) for x in stops)):
        k = np.array([x[min(s, len(x) - 1)] for x in stops], np.int64)
        budget = k + 1 - taken
        steps = env.rollout(policy, episodes=1, max_decisions=budget).cpu().numpy()
        assert np.array_equal(steps, budget), (s, steps, budget)
        taken += budget
        got = _obs(env)
        for b, (name, tr) in enumerate(traces):
            if budget[b] > 0:
                _assert_stored(got, tr, b, int(k[b]), A, T, name)
    fin = H.gpu_final(env)
    for b, (name, tr) in enumerate(traces):
        assert taken[b] == int(tr["n_steps"]) and fin[b]["flags"] & 1, name
        H.assert_final_matches(fin[b], tr, name)


# ---------------------------------------------------------------------------------------------------- 2. the oracle beyond the fixtures
ORACLE_CASES = [
    pytest.param(20, 50, 48, {}, None, id="20A50T-fast"),
    pytest.param(15, 35, 32, {}, ((10, 15), (20, 35)), id="15A35T-ragged-fast"),
    pytest.param(64, 63, 8, {}, None, id="64A63T-fast"),
    pytest.param(64, 64, 6, {}, None, id="64A64T-general-no-depot-lane"),
    pytest.param(70, 130, 6, {}, None, id="70A130T-general"),
    pytest.param(10, 20, 8, dict(member_cap=16), None, id="10A20T-wide-general"),
    pytest.param(4, 700, 2, {}, None, id="4A700T-general-above-64KiB"),        # a launch that needs the raised dynamic-LDS limit
]


@functools.lru_cache(maxsize=None)
def _case_instances(A, T, B, ranges):
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    if ranges is None:
        return generate_batch(B, A, T, base_seed=7000 + 3 * A + T)
    return generate_batch_ranges(range(7100, 7100 + B), *ranges)


@functools.lru_cache(maxsize=None)
def _case_refs(A, T, B, ranges, policy, mwt):
    """Three consecutive oracle episodes of every env of a case (the first one recorded): computed once, shared, never changed."""
    from dcmrta_amd.choice import env_seeds
    inst, seeds = _case_instances(A, T, B, ranges), env_seeds(23, 0, B)
    refs = []
    for b in range(B):
        a, t = (A, T) if ranges is None else (int(inst["n_agents"][b]), int(inst["n_tasks"][b]))
        one = O.one(inst, b, t)
        eps = O.episodes(a, t, one, seeds[b], policy, 3, mwt)
        first = O.episodes(a, t, one, seeds[b], policy, 1, mwt, record=True)[0]
        refs.append((a, t, eps, first))
    return seeds, refs


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("A,T,B,kw,ranges", ORACLE_CASES)
def test_three_episodes_and_a_random_stop_against_the_oracle(gpu_device, A, T, B, kw, ranges, policy):
    """Per env: a stop at a random decision of the first episode (max_decisions_in) against the oracle's recorded observation of that
    decision; then, on a fresh reset, three consecutive episodes in one launch -- return log, steps, summary rows, task / agent getters
    of the third episode."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    inst = _case_instances(A, T, B, ranges)
    seeds, refs = _case_refs(A, T, B, ranges, policy, kw.get("max_waiting_time", 10.0))
    env = BatchedTaskEnv(B, A, T, device=gpu_device, **kw)
    if T == 700:
        assert env.record_bytes() > 65536
    if ranges is None:
        env.load_instances(**inst)
    else:                                                # per-env sizes drawn on the device; the oracle plays the host generator's batch
        env.generate_instances(np.arange(7100, 7100 + B, dtype=np.uint64), agents_range=ranges[0], tasks_range=ranges[1])
        assert np.array_equal(env.n_agents, inst["n_agents"]) and np.array_equal(env.n_tasks, inst["n_tasks"])
        assert len(set(zip(inst["n_agents"].tolist(), inst["n_tasks"].tolist()))) > B // 2
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    rng = np.random.default_rng(A * 131 + T + len(policy))
    at = np.array([rng.integers(1, r[3]["n_steps"] + 1) for r in refs], np.int64)          # decisions taken: 1 .. n
    steps = env.rollout(policy, episodes=1, max_decisions=at).cpu().numpy()
    assert np.array_equal(steps, at)
    got = _obs(env)
    ag, tk, mk = got
    for b, (a, t, _, first) in enumerate(refs):
        _assert_stored(got, first, b, int(at[b]) - 1, a, t, f"{A}A{T}T {policy}")
        if ranges is not None:                                                              # padding rows in the policy's convention
            assert (ag[b, a:] == -1).all() and (tk[b, t + 1:] == -1).all() and mk[b, t + 1:].all(), b
    env.reset(seeds, observe=False)
    steps = env.rollout(policy, episodes=3).cpu().numpy()
    rl, sm, fin = ring.cpu().numpy(), env.summary().cpu().numpy(), H.gpu_final(env)
    for b, (a, t, eps, _) in enumerate(refs):
        tag = f"{A}A{T}T {policy} env{b}"
        assert steps[b] == sum(e["n_steps"] for e in eps), tag
        assert np.array_equal(rl[b], np.array([e["reward"] for e in eps])), tag
        assert np.array_equal(sm[b], O.summary_row(eps[-1])), tag
        f = dict(fin[b])
        for k in ("finished", "feasible", "time_start", "time_finish", "task_wait", "n_members", "n_abandoned"):
            f[k] = f[k][:t]
        for k in ("travel_dist", "returned", "agent_wait"):
            f[k] = f[k][:a]
        H.assert_final_matches(f, eps[-1], tag)


@pytest.mark.parametrize("policy", POLICIES)
def test_wide_handle_above_64KiB_against_the_oracle(gpu_device, policy):
    """The same comparison on a wide handle (sixteen member slots) at the smallest T whose record no longer fits the default 64 KiB
    of dynamic LDS; T comes from the sizes the library reports."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    A, B, kw = 4, 2, dict(member_cap=16)
    size = lambda t: BatchedTaskEnv(B, A, t, device=gpu_device, **kw).record_bytes()
    lo, hi = 1, 2                                        # size(lo) <= 65536 < size(hi)
    while size(hi) <= 65536:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if size(mid) > 65536 else (mid, hi)
    assert size(hi - 1) <= 65536 < size(hi)
    test_three_episodes_and_a_random_stop_against_the_oracle(gpu_device, A, hi, B, kw, None, policy)


@pytest.mark.parametrize("policy", POLICIES)
def test_zero_max_waiting_time_under_a_budget(gpu_device, policy):
    """A max_waiting_time = 0 handle at 20A/50T, B = 8 (the general form).  The issue asked for three full episodes here; under a greedy
    policy they do not exist: a member that has waited 0 is dropped at once (env/task_env.py:269), decides again at the same `now` and
    takes the same task again -- the oracle itself runs past 3 000 000 decisions of env 0 at a constant clock (3.43 under `first`, 0.69
    under `nearest`, measured with this file's instances).  So the launch is refused without a decision budget, and with one every env is
    compared with the oracle's first N decisions: a stop at a random decision (max_decisions_in), then the stop after decision N -- the
    kernel's stores, the decision counter, the clock, and the task / agent getters of the state reached (the waiting sums are
    terminal quantities and no episode ends; summary rows stay NaN, the return log empty)."""
    import oracle
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd._lib import DcmError
    from dcmrta_amd.choice import env_seeds
    A, T, B, N = 20, 50, 8, 400
    inst, seeds = _case_instances(A, T, B, None), env_seeds(23, 0, B)
    refs = [oracle.OracleEnv(A, T, max_waiting_time=0.0).load(inst["depot"][b], inst["task_xy"][b], inst["req"][b], inst["dur"][b])
            .rollout(int(seeds[b]), 0, O.opol(policy), cap_steps=N, record=True, allow_cap=True) for b in range(B)]
    assert all(r["n_steps"] == N for r in refs)
    env = BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=0.0).load_instances(**inst)
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    with pytest.raises(DcmError, match="give a decision budget"):
        env.rollout(policy, episodes=3)
    # a negative ("no limit") entry of max_decisions_in counts as 0 on such a handle: the env takes no decision, nothing spins
    before = env.clone_state().cpu().numpy().copy()
    neg = np.array([-1, 0, -5, -1, 0, -1, -(1 << 40), -1], np.int64)
    assert np.array_equal(env.rollout(policy, episodes=3, max_decisions=neg).cpu().numpy(), np.zeros(B, np.int64))
    assert np.array_equal(env.clone_state().cpu().numpy(), before)
    at = np.random.default_rng(len(policy)).integers(1, N // 2, B).astype(np.int64)
    assert np.array_equal(env.rollout(policy, episodes=3, max_decisions=at).cpu().numpy(), at)
    got = _obs(env)
    for b in range(B):
        _assert_stored(got, refs[b], b, int(at[b]) - 1, A, T, f"mwt0 {policy}")
    assert np.array_equal(env.rollout(policy, episodes=3, max_decisions=N - at).cpu().numpy(), N - at)
    got, st, fin = _obs(env), {k: v.cpu().numpy() for k, v in env.status().items()}, H.gpu_final(env)
    assert np.isnan(env.summary().cpu().numpy()).all() and np.isnan(ring.cpu().numpy()).all()
    for b in range(B):
        _assert_stored(got, refs[b], b, N - 1, A, T, f"mwt0 {policy}")
        assert st["decisions"][b] == N and st["now"][b] == refs[b]["now"][N - 1] and not (st["flags"][b] & 1), b
        for k in ("finished", "feasible", "time_start", "time_finish", "n_members", "n_abandoned", "travel_dist", "returned"):
            assert np.array_equal(np.asarray(fin[b][k]).astype(np.asarray(refs[b][k]).dtype), refs[b][k]), (b, k)


# ---------------------------------------------------------------------------------------------------- 3. ties and rounding (nearest)
DEPOT = np.array([0.5, 0.5])


def _sq_fma(ax, ay, bx, by):
    """fma(dy, dy, dx * dx) as the project's distance routine forms it (agent first), exactly: one rounding of dy^2 + RN(dx^2)."""
    from fractions import Fraction
    dx, dy = ax - bx, ay - by
    return float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx))


def _dist(ax, ay, bx, by):
    return float(np.sqrt(np.float64(_sq_fma(ax, ay, bx, by))))


def _rounding_pairs(want=8):
    """Pairs of points whose SQUARED distances from the depot differ -- formed with the fused multiply-add and without -- while
    np.linalg.norm (and the square root of either square) rounds both to the same double; returned with the larger square first.
    The second point is the first with its y moved one ulp away from the depot, |dy| << |dx|: the square then moves by about one
    ulp, and roughly two adjacent squares share a root.  The search keeps only what it has checked."""
    rng = np.random.default_rng(2024)
    pairs = []
    for _ in range(20000):
        p = DEPOT + np.array([rng.uniform(0.15, 0.3), rng.uniform(0.02, 0.08)]) * rng.choice([-1.0, 1.0], 2)
        q = np.array([p[0], np.nextafter(p[1], 2.0 if p[1] > DEPOT[1] else -1.0)])
        fsq = [_sq_fma(DEPOT[0], DEPOT[1], r[0], r[1]) for r in (p, q)]
        psq = [float((DEPOT[0] - r[0]) * (DEPOT[0] - r[0]) + (DEPOT[1] - r[1]) * (DEPOT[1] - r[1])) for r in (p, q)]
        same_root = np.linalg.norm(DEPOT - p) == np.linalg.norm(DEPOT - q) and np.sqrt(fsq[0]) == np.sqrt(fsq[1]) and \
            np.sqrt(psq[0]) == np.sqrt(psq[1])
        if fsq[1] > fsq[0] and psq[1] > psq[0] and same_root:
            pairs.append((q, p))
            if len(pairs) == want:
                break
    return pairs


SMALL_TIES = [(2, 5, 7), (0, 1, 2), (9, 11), (3, 6, 8)]
SMALL_PAIRS = [((e * 3) % 11, (e * 3) % 11 + 1) for e in range(4, 12)]
# more than one lane chunk of tasks (task t: lane t % 64 of chunk t // 64): the lowest index sits in a HIGHER lane than another candidate
# (70 / 129, 65 / 128), in the same lane (5 / 69), next to a chunk boundary (63 / 64 / 127); the pairs likewise
CHUNK_TIES = [(70, 129), (5, 69, 128), (63, 64, 127), (65, 128, 129)]
CHUNK_PAIRS = [(10, 74), (11, 74), (70, 129), (0, 128), (63, 64), (1, 65), (37, 100), (127, 128)]
# form: A, T, tied index sets of env 0..3, (lower, higher) indices of the rounding pairs of env 4..11
TIE_FORMS = {
    "fast": (6, 12, SMALL_TIES, SMALL_PAIRS),
    "general-partial-obs": (6, 12, SMALL_TIES, SMALL_PAIRS),                # the one-chunk branch of Sim::pick_policy_action
    "general-multi-chunk": (6, 130, CHUNK_TIES, CHUNK_PAIRS),               # Sim<128,256,runtime>: three chunks, coordinates in LDS
    "general-50A200T": (50, 200, CHUNK_TIES, CHUNK_PAIRS),                  # Sim<50,200>: four chunks, coordinates in registers
}


def _tie_instances(T, ties, pair_idx):
    """B instances, all agents at the depot (0.5, 0.5) at the first decision.  Env 0..2: mirror images at equal, exactly representable
    distance 0.25 in the tasks of ties[e], everything else farther.  Env 3: the same with requirement 1 on the lowest candidate, so
    that its coalition completes with the first join and the next candidate takes over.  Env 4..: one rounding pair each, the lower
    index holding the LARGER square, everything else farther."""
    mirrors = [np.array([0.25, 0.5]), np.array([0.75, 0.5]), np.array([0.5, 0.25]), np.array([0.5, 0.75])]
    far = lambda rng: DEPOT + rng.uniform(0.35, 0.49, 2) * rng.choice([-1.0, 1.0], 2)      # > 0.35 from the depot on each axis
    rng = np.random.default_rng(5)
    out, expect = [], []
    pairs = _rounding_pairs()
    assert len(pairs) >= 8, len(pairs)
    assert len(pair_idx) == len(pairs) == 8 and all(lo < hi < T for lo, hi in pair_idx) and all(list(t) == sorted(t) for t in ties)
    for e in range(4 + len(pairs)):
        xy = np.stack([far(rng) for _ in range(T)])
        req = rng.integers(2, 4, T).astype(np.int32)
        if e < 4:
            idx = ties[e]
            for j, t in enumerate(idx):
                xy[t] = mirrors[j]
            if e == 3:
                req[idx[0]] = 1
            expect.append(idx)
        else:
            big, small = pairs[e - 4]
            lo, hi = pair_idx[e - 4]
            xy[lo], xy[hi] = big, small
            expect.append((lo, hi))
        out.append(dict(depot=DEPOT.copy(), task_xy=xy, req=req, dur=np.full(T, 2.0)))
    return out, expect


@pytest.mark.parametrize("form", sorted(TIE_FORMS))
def test_nearest_ties_go_to_the_lowest_index_and_roots_are_compared(gpu_device, form):
    """(a) equal distances: the lowest index wins, and once it is masked the next one; (b) different squares under one rounded root:
    the lower index wins although its square is the larger one (a kernel that compares squares takes the other).  First decision
    pinned by construction, every later one and the full episode by the oracle.  On the register-resident form, on the general form's
    one-chunk branch (forced by a partial buffer set), and on its multi-chunk argmin with the coordinates in LDS and in registers."""
    import torch
    from dcmrta_amd import _lib
    from dcmrta_amd.batched_env import BatchedTaskEnv, _ptr, check
    from dcmrta_amd.choice import env_seeds
    A, T, ties, pair_idx = TIE_FORMS[form]
    insts, expect = _tie_instances(T, ties, pair_idx)
    B = len(insts)
    mwt = 10.0            # (max_waiting_time = 0 forces the general form too, but a greedy episode does not end there: see above)
    seeds = env_seeds(3, 0, B)
    env = BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=mwt)
    env.load_instances(*[np.stack([i[k] for i in insts]) for k in ("depot", "task_xy", "req", "dur")])
    env.reset(seeds, observe=False)
    refs = [O.episodes(A, T, insts[b], seeds[b], "nearest", 1, mwt, record=True)[0] for b in range(B)]

    def launch(budget):
        if form != "general-partial-obs":
            return env.rollout("nearest", episodes=1, max_decisions=budget).cpu().numpy()
        steps = torch.empty((B,), dtype=torch.int64, device=env.device)                     # the mask alone: a partial buffer set
        with torch.cuda.device(env.device):
            check(env._lib.dcm_rollout_policy(env._h, _lib.POLICY_NEAREST, 1, int(budget), None, None, None, _ptr(env._mask),
                                              _ptr(steps), env._stream()))
        return steps.cpu().numpy()

    assert np.array_equal(launch(1), np.ones(B, np.int64))
    cur = env.agents_state()["current"].cpu().numpy()
    for b in range(B):
        joined = sorted(set(int(c) for c in cur[b] if c >= 0))
        assert joined == [expect[b][0]], (form, b, joined, expect[b])                       # lowest index of the tied set
        assert int(refs[b]["action"][0]) == expect[b][0] + 1, (form, b)                     # ... and the oracle agrees
    # env 3: requirement 1, so the first join completes the coalition and masks the task; the second decision of the same group (all
    # agents still at the depot) must take the next candidate of the tied set
    assert refs[3]["n_steps"] > 1 and refs[3]["mask"][1][expect[3][0] + 1] == 1 and int(refs[3]["action"][1]) == expect[3][1] + 1
    assert np.array_equal(launch(1), np.ones(B, np.int64))
    cur = env.agents_state()["current"].cpu().numpy()
    assert sorted(set(int(c) for c in cur[3] if c >= 0)) == [expect[3][0], expect[3][1]]
    launch(-1)
    fin = H.gpu_final(env)
    for b in range(B):
        H.assert_final_matches(fin[b], refs[b], f"{form} tie env{b}")


# ---------------------------------------------------------------------------------------------------- 4. renewal
@pytest.mark.parametrize("A,T,B,base", [pytest.param(20, 50, 32, 9100, id="20A50T-fast"), pytest.param(30, 100, 8, 9200, id="30A100T-general")])
def test_nearest_under_instance_renewal(gpu_device, A, T, B, base):
    """Uniform generated batch, stride B, three episodes of `nearest` in one launch: episode k of env e plays instance base + k B + e
    (the host generator) under the running decision counter (the oracle)."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_instance, renewal_seeds
    seeds = env_seeds(61, 0, B)
    env = BatchedTaskEnv(B, A, T, device=gpu_device)
    env.generate_instances(np.arange(base, base + B, dtype=np.uint64))
    env.set_instance_renewal(B)
    ring = env.enable_return_log(3)
    env.reset(seeds, observe=False)
    steps = env.rollout("nearest", episodes=3).cpu().numpy()
    rl, sm, idx, fin = ring.cpu().numpy(), env.summary().cpu().numpy(), env.instance_index().cpu().numpy(), H.gpu_final(env)
    held = {k: v.cpu().numpy() for k, v in env.instances().items() if v is not None}
    for b in range(B):
        assert all(int(renewal_seeds(base + b, k, B)) == base + k * B + b for k in range(3))
        insts = [generate_instance(A, T, int(renewal_seeds(base + b, k, B))) for k in range(3)]
        eps = O.episodes(A, T, insts.__getitem__, seeds[b], "nearest", 3)
        r, inst = eps[-1], insts[-1]
        assert steps[b] == sum(e["n_steps"] for e in eps) and np.array_equal(rl[b], np.array([e["reward"] for e in eps])), b
        assert np.array_equal(sm[b], O.summary_row(r)), b
        assert idx[b] == 2, (b, idx[b])
        assert all(np.array_equal(held[k][b], inst[k]) for k in ("depot", "task_xy", "req", "dur")), b
        H.assert_final_matches(fin[b], r, f"renewal {A}A{T}T env{b}")


@pytest.mark.parametrize("policy", POLICIES)
def test_size_renewing_launch_refuses_a_greedy_policy(gpu_device, policy):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd._lib import DcmError
    B = 8
    env = BatchedTaskEnv(B, 20, 50, device=gpu_device, renew_sizes=True)
    env.generate_instances(np.arange(300, 300 + B, dtype=np.uint64), agents_range=(10, 20), tasks_range=(20, 50))
    env.set_instance_renewal(B)
    env.reset(5, observe=False)
    before = env.clone_state().cpu().numpy().copy()
    with pytest.raises(DcmError, match=r"error %d: dcm_rollout_policy: no greedy policy" % ERR_STATE):
        env.rollout(policy, episodes=2)
    assert np.array_equal(env.clone_state().cpu().numpy(), before)
    env.set_instance_renewal(0)                                                             # ragged without renewal works
    assert int(env.rollout(policy, episodes=1).sum()) > 0


# ---------------------------------------------------------------------------------------------------- 5. interplay
@pytest.mark.parametrize("A,T,B", [(20, 50, 16), (70, 130, 4)])
def test_random_through_the_new_entry_point_is_dcm_rollout_random(gpu_device, A, T, B):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    inst, seeds = generate_batch(B, A, T, base_seed=55), env_seeds(2, 0, B)
    out = []
    for call in ("rollout_random", "rollout"):
        env = BatchedTaskEnv(B, A, T, device=gpu_device).load_instances(**inst)
        env.reset(seeds, observe=False)
        steps = env.rollout_random(episodes=2, max_decisions=150) if call == "rollout_random" else env.rollout("random", episodes=2, max_decisions=150)
        out.append((steps.cpu().numpy(), env.clone_state().cpu().numpy(), env.summary().cpu().numpy(), _obs(env)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2], equal_nan=True)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(out[0][3], out[1][3]))


def _host_pick(policy, mask_row, agents_row_of_leader_xy, tasks_xy):
    """The same rule on the host, from what dcm_observe returns: mask (True = masked) and positions."""
    open_ = np.flatnonzero(~mask_row[1:])
    if len(open_) == 0:
        return 0
    if policy == "first":
        return int(open_[0]) + 1
    d = np.array([_dist(agents_row_of_leader_xy[0], agents_row_of_leader_xy[1], tasks_xy[t][0], tasks_xy[t][1]) for t in open_])
    return int(open_[int(np.argmin(d))]) + 1                                                # argmin: the first minimum


@pytest.mark.parametrize("policy", POLICIES)
def test_budget_stop_leaves_a_valid_decision_point_for_the_lockstep_api(gpu_device, policy):
    """Stop a greedy rollout in mid-episode, finish with dcm_step, the action computed on the host from dcm_observe by the same rule
    (the distance routine restated exactly: _dist): the episode ends with the oracle's results."""
    import torch
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    B, A, T = 6, 20, 50
    inst, seeds = generate_batch(B, A, T, base_seed=808), env_seeds(14, 0, B)
    refs = [O.episodes(A, T, O.one(inst, b), seeds[b], policy, 1)[0] for b in range(B)]
    env = BatchedTaskEnv(B, A, T, device=gpu_device).load_instances(**inst)
    env.reset(seeds, observe=False)
    at = np.array([max(1, r["n_steps"] // 3) for r in refs], np.int64)
    assert np.array_equal(env.rollout(policy, episodes=1, max_decisions=at).cpu().numpy(), at)
    obs = env.observe()
    taken = at.copy()
    for _ in range(400):
        active = obs.active.cpu().numpy()
        if not active.any():
            break
        mask, leader = obs.mask.cpu().numpy(), obs.leader.cpu().numpy()
        ag = env.agents_state()
        x, y = ag["x"].cpu().numpy(), ag["y"].cpu().numpy()
        actions = np.zeros(B, np.int32)
        for b in np.flatnonzero(active):
            actions[b] = _host_pick(policy, mask[b], np.array([x[b, leader[b]], y[b, leader[b]]]), inst["task_xy"][b])
        taken += active
        obs = env.step(torch.from_numpy(actions).to(env.device))
    assert not obs.active.cpu().numpy().any()
    fin = H.gpu_final(env)
    for b in range(B):
        assert taken[b] == refs[b]["n_steps"], (b, taken[b], refs[b]["n_steps"])
        H.assert_final_matches(fin[b], refs[b], f"{policy} handover env{b}")


def test_unknown_policy_is_invalid(gpu_device):
    import torch
    from dcmrta_amd.batched_env import BatchedTaskEnv, _ptr
    from dcmrta_amd.instances import generate_batch
    B = 4
    env = BatchedTaskEnv(B, 20, 50, device=gpu_device).load_instances(**generate_batch(B, 20, 50, base_seed=1))
    env.reset(1, observe=False)
    before = env.clone_state().cpu().numpy().copy()
    steps = torch.full((B,), -7, dtype=torch.int64, device=env.device)
    for bad in (3, -1, 99):
        with torch.cuda.device(env.device):
            rc = env._lib.dcm_rollout_policy(env._h, bad, 1, -1, None, None, None, None, _ptr(steps), env._stream())
        assert rc == ERR_INVALID and b"unknown policy" in env._lib.dcm_last_error()
    assert (steps.cpu().numpy() == -7).all() and np.array_equal(env.clone_state().cpu().numpy(), before)
    with pytest.raises(Exception, match="policy must be one of"):
        env.rollout("greedy")
