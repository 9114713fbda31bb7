"""Episode boundaries inside one persistent launch: an episode that another one of the same unbudgeted call follows ends without its
terminal metrics (nobody can read them: the next terminal rewrites the summary row and the metrics' scratch, the restart clears the
flags).  Nothing a caller can see may depend on that: a call of N episodes leaves what N calls of one episode leave -- every episode of
a one-episode call is the call's last, so it computes its metrics -- and what the oracle computes.  A budgeted call skips nothing: its
summary row is the last FINISHED episode's wherever the budget stops it.  The best-keeping form reads the row behind every finished
episode and keeps the metrics.

Shapes: 64 envs of 6A/3T, 64 of 20A/50T, 64 of 15A/35T on a ragged 20A/50T handle (the runtime-size layout of the one-chunk kernel),
16 envs of 50A/200T and of 70A/130T (the multi-chunk families).  generate_batch(..., base_seed=1), env_seeds(1, 0, B)."""
import numpy as np
import pytest

import oracle_ref as O
import renewal_ref as R

EP_MAX = 4
#                  A,  T,  B, env's own (a, t) on a ragged handle
CASES = {"6A3T": (6, 3, 64, None),
         "20A50T": (20, 50, 64, None),
         "15A35T_ragged": (20, 50, 64, (15, 35)),
         "50A200T": (50, 200, 16, None),
         "70A130T": (70, 130, 16, None)}
ONE_CHUNK = ["6A3T", "20A50T", "15A35T_ragged"]
UNIFORM = ["6A3T", "20A50T"]
MULTI_CHUNK = ["50A200T", "70A130T"]

_inputs, _oracle = {}, {}


def inputs(name):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    if name not in _inputs:
        A, T, B, own = CASES[name]
        inst = generate_batch(B, A, T, base_seed=1)
        if own:
            inst = dict(inst, n_agents=np.full(B, own[0], np.int32), n_tasks=np.full(B, own[1], np.int32))
        _inputs[name] = (inst, env_seeds(1, 0, B))
    return _inputs[name]


def oracle_episodes(name, policy="random"):
    """EP_MAX consecutive oracle episodes of every env (computed once, read-only afterwards)"""
    if (name, policy) not in _oracle:
        A, T, B, own = CASES[name]
        a, t = own or (A, T)
        inst, seeds = inputs(name)
        _oracle[name, policy] = [O.episodes(a, t, O.one(inst, b, t), seeds[b], policy, EP_MAX) for b in range(B)]
    return _oracle[name, policy]


def make(gpu_device, name, ring=3, **kw):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    A, T, B, _ = CASES[name]
    inst, seeds = inputs(name)
    env = BatchedTaskEnv(B, A, T, device=gpu_device, **kw).load_instances(**inst)
    r = env.enable_return_log(ring)
    env.reset(seeds, observe=False)
    return env, r


def everything(env, ring, with_obs):
    """All a caller can read after a call, as named byte arrays"""
    out = dict(summary=env.summary(), ring=ring, episodes=env.episodes(), clone_state=env.clone_state())
    out.update({"status." + k: v for k, v in env.status().items()})
    out.update({"tasks." + k: v for k, v in env.tasks_state().items()})
    out.update({"agents." + k: v for k, v in env.agents_state().items()})
    if with_obs:
        o = env.obs()
        out.update(obs_agents=o.agents, obs_tasks=o.tasks, obs_mask=o.mask)
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (tag, k)
        bad = np.flatnonzero(a[k].reshape(-1).view(np.uint8) != b[k].reshape(-1).view(np.uint8))
        assert bad.size == 0, (tag, k, "first differing bytes", bad[:8].tolist())


def one_call_equals_n(gpu_device, name, policy, n, write_obs):
    one, ring1 = make(gpu_device, name)
    many, ringn = make(gpu_device, name)
    s1 = one.rollout(policy, episodes=n, write_obs=write_obs).cpu().numpy()
    sn = sum(many.rollout(policy, episodes=1, write_obs=write_obs).cpu().numpy() for _ in range(n))
    assert s1.sum() > 0 and np.array_equal(s1, sn), (name, policy, n, "steps")
    assert (one.episodes().cpu().numpy() == n).all()
    assert_same(everything(one, ring1, write_obs), everything(many, ringn, write_obs), (name, policy, n, write_obs))
    one.close(); many.close()
    return s1


@pytest.mark.gpu
@pytest.mark.parametrize("write_obs", [True, False])
@pytest.mark.parametrize("n", [3, 2, 4])
@pytest.mark.parametrize("name", ONE_CHUNK)
def test_one_call_equals_n_calls(gpu_device, name, n, write_obs):
    one_call_equals_n(gpu_device, name, "random", n, write_obs)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["first", "nearest"])
@pytest.mark.parametrize("name", ONE_CHUNK)
def test_one_call_equals_three_calls_greedy(gpu_device, name, policy):
    one_call_equals_n(gpu_device, name, policy, 3, True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MULTI_CHUNK)
def test_one_call_equals_three_calls_multi_chunk(gpu_device, name):
    one_call_equals_n(gpu_device, name, "random", 3, True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNIFORM)
def test_three_episodes_against_the_oracle(gpu_device, oracle_lib, name):
    """As bench.py's parity_rollout: steps, every episode's return, the last episode's reward, finished-task count and six metrics"""
    A = CASES[name][0]
    inst, seeds = inputs(name)
    env, ring = make(gpu_device, name)
    steps = env.rollout_random(episodes=3).cpu().numpy()
    sm, got = env.summary().cpu().numpy(), ring.cpu().numpy()
    ref = oracle_lib.batch_rollout_full(inst["depot"], inst["task_xy"], inst["req"], inst["dur"], seeds, A, episodes=3, threads=4)
    bits = lambda x, y: np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert bits(steps, ref["steps"]), name
    assert bits(got, ref["returns"]), name
    assert bits(sm[:, 0], ref["reward"]) and bits(sm[:, 1].astype(np.int32), ref["n_finished"]) and bits(sm[:, 2:8], ref["metrics"]), name
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mid_episode_2", "own_episode_1", "one"])
@pytest.mark.parametrize("name", ONE_CHUNK)
def test_budgets_keep_every_finished_episode(gpu_device, oracle_lib, name, kind):
    """A budgeted three-episode call, then a call that plays every env on to the end of its third episode.  After the first: the summary
    row is the oracle's row of the last episode the env has FINISHED (an episode whose last decision is the budget's last counts).
    After the second, in every env: everything equals the unbudgeted call's, clone_state() byte for byte."""
    B = CASES[name][2]
    eps = oracle_episodes(name)
    n = np.array([[r["n_steps"] for r in e] for e in eps], np.int64)            # [B, EP_MAX]
    if kind == "mid_episode_2":
        # the int that puts the most envs inside their second episode: past the first, at least one decision short of the second's end
        cands = np.arange(int(n[:, 0].min()) + 1, int((n[:, 0] + n[:, 1]).max()))
        budget = int(cands[np.argmax([((n[:, 0] < c) & (c < n[:, 0] + n[:, 1])).sum() for c in cands])])
        per_env = np.full(B, budget, np.int64)
    elif kind == "own_episode_1":
        budget = per_env = n[:, 0].copy()
    else:
        budget, per_env = 1, np.ones(B, np.int64)
    cum = np.cumsum(n[:, :3], axis=1)
    finished = (cum <= per_env[:, None]).sum(axis=1)                             # episodes finished within the budget
    if kind == "mid_episode_2":
        print(name, "budget", budget, "envs stopped inside episode 2:", int(((finished == 1) & (per_env > cum[:, 0])).sum()), "of", B)
        assert ((finished == 1) & (per_env > cum[:, 0])).sum() >= B // 2
    elif kind == "own_episode_1":
        assert (finished == 1).all()
    env, ring = make(gpu_device, name)
    steps = env.rollout_random(episodes=3, max_decisions=budget).cpu().numpy()
    assert np.array_equal(steps, np.minimum(per_env, cum[:, 2])), (name, kind)
    sm, got = env.summary().cpu().numpy(), ring.cpu().numpy()
    assert np.array_equal(env.episodes().cpu().numpy(), finished), (name, kind)
    for b in range(B):
        for k in range(finished[b]):
            assert got[b, k] == eps[b][k]["reward"], (name, kind, b, k)
        if finished[b]:
            O.assert_summary(sm[b], eps[b][finished[b] - 1], f"{name} {kind} env {b} after episode {finished[b]}")
    # the continuation, per env: three more episode slots (more than any env needs) under the budget that is left of its three episodes,
    # so every env stops with the last decision of its third episode -- where the unbudgeted call stands
    steps2 = env.rollout_random(episodes=3, max_decisions=cum[:, 2] - steps).cpu().numpy()
    ref, ref_ring = make(gpu_device, name)
    ref_steps = ref.rollout_random(episodes=3).cpu().numpy()
    assert np.array_equal(steps + steps2, ref_steps) and np.array_equal(ref_steps, cum[:, 2]), (name, kind)
    assert_same(everything(env, ring, True), everything(ref, ref_ring, True), (name, kind, "continued"))
    env.close(); ref.close()


@pytest.mark.gpu
def test_logging_form_three_episodes(gpu_device, oracle_lib):
    """The rollout log on: everything equals the plain three-episode call, and the log holds the oracle's third episode"""
    name = "20A50T"
    A, T, B, _ = CASES[name]
    inst, seeds = inputs(name)
    plain, ring0 = make(gpu_device, name)
    logged, ring1 = make(gpu_device, name)
    logged.enable_rollout_log(64)
    logged.reset(seeds, observe=False)
    s0, s1 = plain.rollout_random(episodes=3).cpu().numpy(), logged.rollout_random(episodes=3).cpu().numpy()
    assert np.array_equal(s0, s1)
    assert_same(everything(plain, ring0, True), everything(logged, ring1, True), "logging form")
    log = O.log(logged)
    for b in range(0, B, 8):
        sim = O.Sim(A, T, lambda j, b=b: O.one(inst, b), seeds[b], "random")
        assert sim.launch(3, -1) == s1[b]
        O.assert_log(log, b, sim, "three episodes")
    plain.close(); logged.close()


@pytest.mark.gpu
def test_best_keeping_form_three_episodes(gpu_device):
    """The best log on (this form reads the summary row behind every finished episode and keeps its metrics): the kept row is the best
    of the three rows that three one-episode calls show -- by (finished tasks, reward), the earliest on a tie"""
    name = "20A50T"
    B = CASES[name][2]
    _, seeds = inputs(name)
    rows = []
    single, _ = make(gpu_device, name)
    for _ in range(3):
        single.rollout_random(episodes=1)
        rows.append(single.summary().cpu().numpy().copy())
    best, ring = make(gpu_device, name)
    best.enable_rollout_log(64)
    best.enable_best_log()
    best.reset(seeds, observe=False)
    best.rollout_random(episodes=3)
    kept, which = best.best_summary().cpu().numpy(), best.best_episode().cpu().numpy()
    for b in range(B):
        k = max(range(3), key=lambda i: (rows[i][b, 1], rows[i][b, 0], -i))
        assert which[b] == k and np.array_equal(kept[b].view(np.uint64), rows[k][b].view(np.uint64)), (b, which[b], k)
    assert np.array_equal(best.summary().cpu().numpy().view(np.uint64), rows[2].view(np.uint64))
    single.close(); best.close()


@pytest.mark.gpu
def test_renewing_form_three_episodes(gpu_device, oracle_lib):
    """Instance renewal on (stride B): episode k of env b plays the host generator's instance base + k B + b"""
    B, base = 16, 7300
    seeds = inputs("20A50T")[1][:B]
    env, ring = R.make(gpu_device, B, 20, 50, base, B)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=R.EPISODES).cpu().numpy()
    R.assert_after(env, ring, R.chains(20, 50, B, base, B, seeds), steps)
    env.close()
