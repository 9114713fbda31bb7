"""-m gpu: problem instances made on the device (dcm_generate_instances, csrc/instgen.hpp + np_stream.hpp) are bit-equal to the host
generators of dcmrta_amd/instances.py, i.e. to TaskEnv(agents_range, tasks_range, max_coalition_size, seed=s) of the reference
(env/task_env.py:57-71; tests/golden/instgen.npz), and a handle filled that way behaves exactly like one filled by load_instances.
Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers as H
from fixtures_ref import BIG_SEEDS, assert_same_instances, held_instances, replay_recorded
from renewal_ref import first_valid

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ 1. known answers of the stream
@pytest.mark.parametrize("bound", [5, 3 * 2 ** 30, 2 ** 32 - 1])
def test_generator_draws_equal_numpy(gpu_device, bound):
    """Generator.random then Generator.integers(0, bound) for 4096 seeds x (64 doubles, 64 ints).  At 3 * 2^30 a quarter of the
    words is rejected, so practically every wave leaves the jump-ahead path for the sequential routine; at 5 practically none."""
    from dcmrta_amd.batched_env import device_generator_draws
    seeds = np.concatenate([np.arange(4096 - len(BIG_SEEDS), dtype=np.uint64), np.array(BIG_SEEDS, dtype=np.uint64)])
    d, i = device_generator_draws(seeds, 64, bound, 64, device=gpu_device)
    assert d.shape == (4096, 64) and i.shape == (4096, 64) and i.dtype == np.uint32
    for n, s in enumerate(seeds):
        g = np.random.default_rng(int(s))
        assert np.array_equal(d[n], g.random(64)), (bound, s)
        assert np.array_equal(i[n], g.integers(0, bound, 64).astype(np.uint32)), (bound, s)


def test_generator_draws_odd_counts_and_long_runs(gpu_device):
    """Counts that are no multiple of the wave, no doubles at all, and runs of several 128-word blocks."""
    from dcmrta_amd.batched_env import device_generator_draws
    seeds = np.array(list(range(40)) + BIG_SEEDS, dtype=np.uint64)
    for nd, bound, ni in ((0, 7, 1), (1, 16, 127), (3, 16, 129), (65, 1000, 500), (130, 1, 9), (7, 2 ** 31 + 1, 300)):
        d, i = device_generator_draws(seeds, nd, bound, ni, device=gpu_device)
        for n, s in enumerate(seeds):
            g = np.random.default_rng(int(s))
            assert np.array_equal(d[n], g.random(nd)) and np.array_equal(i[n], g.integers(0, bound, ni).astype(np.uint32)), (nd, bound, ni, s)


# ------------------------------------------------------------------ 2. generated batches
@pytest.mark.parametrize("shape", [(5, 8), (20, 50), (64, 64), (50, 200), (100, 500)])
def test_uniform_batch_equals_generate_batch(gpu_device, shape):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.instances import generate_batch
    A, T = shape
    B = 96
    env = BatchedTaskEnv(B, A, T, device=gpu_device)
    assert env.generate_instances(1000) is env and env.n_agents is None and env.n_tasks is None
    assert_same_instances(held_instances(env), generate_batch(B, A, T, base_seed=1000), shape)
    # other requirement range and duration; seeds as an array, and as a torch tensor, incl. seeds >= 2^32 and >= 2^63
    seeds = np.array(list(range(7, 7 + B - len(BIG_SEEDS))) + BIG_SEEDS, dtype=np.uint64)
    want = generate_batch(B, A, T, max_coalition_size=3, max_duration=2.5)
    for b, s in enumerate(seeds):
        one = generate_batch(1, A, T, base_seed=int(s), max_coalition_size=3, max_duration=2.5)
        for k in want:
            want[k][b] = one[k][0]
    env.generate_instances(seeds, max_coalition_size=3, max_duration=2.5)
    assert_same_instances(held_instances(env), want, shape)
    env.generate_instances(torch.from_numpy(seeds.view(np.int64)).to(gpu_device), A, (T, T), 3, 2.5)
    assert_same_instances(held_instances(env), want, shape)


def test_wide_handle_at_sixteen(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    B, A, T = 64, 20, 50
    env = BatchedTaskEnv(B, A, T, device=gpu_device, member_cap=16).generate_instances(300, max_coalition_size=16)
    want = generate_batch(B, A, T, base_seed=300, max_coalition_size=16)
    assert want["req"].max() == 16
    assert_same_instances(held_instances(env), want)
    env.generate_instances(300, (10, 20), (20, 50), max_coalition_size=16)
    assert_same_instances(held_instances(env), generate_batch_ranges(range(300, 300 + B), (10, 20), (20, 50), max_coalition_size=16))


@pytest.mark.parametrize("ranges", [((10, 20), (20, 50)), (15, (20, 50)), ((10, 20), 40), ((3, 128), (1, 300)), ((20, 20), (50, 50)),
                                    (12, 30)])
def test_ragged_batch_equals_generate_batch_ranges(gpu_device, ranges):
    """Both sizes drawn, one of them (the first requirement then takes the half-word the size left behind), none -- on a handle
    whose dims are the range maxima, and on a larger 20A/50T-layout handle (a range that is an int below the handle's dim)."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.instances import generate_batch_ranges
    ar, tr = ranges
    A, T = (ar[1] if isinstance(ar, tuple) else ar), (tr[1] if isinstance(tr, tuple) else tr)
    B = 128
    seeds = np.array(list(range(500, 500 + B - len(BIG_SEEDS))) + BIG_SEEDS, dtype=np.uint64)
    for m in (1, 3, 5):
        want = generate_batch_ranges([int(s) for s in seeds], ar, tr, max_coalition_size=m)
        env = BatchedTaskEnv(B, A, T, device=gpu_device).generate_instances(seeds, ar, tr, max_coalition_size=m)
        uniform = not (isinstance(ar, tuple) and ar[0] != ar[1]) and not (isinstance(tr, tuple) and tr[0] != tr[1])
        if uniform:
            assert env.n_agents is None and env.n_tasks is None
            want["n_agents"] = want["n_tasks"] = None
        else:
            assert np.array_equal(env.n_agents, want["n_agents"]) and np.array_equal(env.n_tasks, want["n_tasks"])
        assert_same_instances(held_instances(env), want, (ranges, m))
    if A <= 18 and T <= 45:
        env = BatchedTaskEnv(B, 20, 50, device=gpu_device).generate_instances(seeds, ar, tr)
        got, want = held_instances(env), generate_batch_ranges([int(s) for s in seeds], ar, tr)
        assert np.array_equal(got["n_agents"], want["n_agents"]) and np.array_equal(got["task_xy"][:, :T], want["task_xy"])
        assert np.array_equal(got["req"][:, :T], want["req"]) and (got["req"][:, T:] == 1).all() and not got["task_xy"][:, T:].any()


def test_reference_golden_instances(gpu_device, golden_dir):
    """Every case of tests/golden/instgen.npz, written by the reference's own TaskEnv."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    z = np.load(os.path.join(golden_dir, "instgen.npz"))
    assert len(z["cases"]) >= 15
    for name in z["cases"]:
        a_lo, a_hi, a_tuple, t_lo, t_hi, t_tuple, m = (int(x) for x in z[f"{name}/params"])
        seeds = z[f"{name}/seeds"]
        env = BatchedTaskEnv(len(seeds), a_hi, t_hi, device=gpu_device, member_cap=m)
        env.generate_instances(seeds, (a_lo, a_hi) if a_tuple else a_lo, (t_lo, t_hi) if t_tuple else t_lo, max_coalition_size=m, max_duration=5)
        got = held_instances(env)
        for k in ("depot", "task_xy", "req", "dur"):
            assert np.array_equal(got[k], z[f"{name}/{k}"]), (name, k)
        if a_lo != a_hi or t_lo != t_hi:
            assert np.array_equal(got["n_agents"], z[f"{name}/n_agents"]) and np.array_equal(got["n_tasks"], z[f"{name}/n_tasks"]), name
        else:
            assert got["n_agents"] is None and (z[f"{name}/n_agents"] == a_hi).all() and (z[f"{name}/n_tasks"] == t_hi).all(), name


def test_instances_getter_returns_loaded_instances(gpu_device):
    """instances() returns what the handle holds however it got there: a host-loaded uniform and a host-loaded ragged batch."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    B, A, T = 32, 20, 50
    inst = generate_batch(B, A, T, base_seed=4)
    env = BatchedTaskEnv(B, A, T, device=gpu_device).load_instances(**inst)
    assert_same_instances(held_instances(env), inst)
    rag = generate_batch_ranges(range(B), (10, 20), (20, 50))
    env.load_instances(**rag)
    assert_same_instances(held_instances(env), rag)


# ------------------------------------------------------------------ 3. a generated handle behaves like a host-loaded twin
def _twin_state(env, seeds, episodes=2):
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=episodes)
    obs = env.obs()
    return dict(steps=steps, summary=env.summary(), flags=env.status()["flags"], decisions=env.status()["decisions"],
                agents=obs.agents.clone(), tasks=obs.tasks.clone(), mask=obs.mask.clone())


@pytest.mark.parametrize("case", ["20A50T", "ragged", "50A200T"])
def test_rollout_equals_host_loaded_twin(gpu_device, case):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    B = 128
    A, T = (50, 200) if case == "50A200T" else (20, 50)
    seeds = env_seeds(17, 0, B)
    if case == "ragged":
        dev_env = BatchedTaskEnv(B, A, T, device=gpu_device).generate_instances(40, (10, 20), (20, 50))
        inst = generate_batch_ranges(range(40, 40 + B), (10, 20), (20, 50))
    else:
        dev_env = BatchedTaskEnv(B, A, T, device=gpu_device).generate_instances(40)
        inst = generate_batch(B, A, T, base_seed=40)
    twin = BatchedTaskEnv(B, A, T, device=gpu_device).load_instances(**inst)
    got, want = _twin_state(dev_env, seeds), _twin_state(twin, seeds)
    assert int(want["steps"].sum()) > 2 * B
    for k in want:
        assert torch.equal(got[k], want[k]), (case, k)


def test_generated_batch_matches_oracle_env_by_env(gpu_device, oracle_lib):
    """256 envs of 20A/50T made on the device, one random-policy episode each: every env against the oracle fed with the HOST
    generator's instance, as smoke() does."""
    import oracle
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    B, A, T = 256, 20, 50
    inst = generate_batch(B, A, T, base_seed=42)
    seeds = env_seeds(42, 0, B)
    env = BatchedTaskEnv(B, A, T, device=gpu_device).generate_instances(42)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=1).cpu().numpy()
    fin = H.gpu_final(env)
    sm = env.summary().cpu().numpy()
    for b in range(B):
        ref = oracle.OracleEnv(A, T).load(inst["depot"][b], inst["task_xy"][b], inst["req"][b], inst["dur"][b]) \
            .rollout(int(seeds[b]), 0, oracle.POLICY_RANDOM, record=False)
        assert steps[b] == ref["n_steps"] and sm[b, 0] == ref["reward"], b
        H.assert_final_matches(fin[b], ref, f"env {b}")


def test_route_replay_equals_host_loaded_twin(gpu_device):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.instances import generate_batch, synthetic_route_arrays
    B, A, T = 64, 20, 50
    inst = generate_batch(B, A, T, base_seed=9)
    routes, lens = synthetic_route_arrays(inst["req"], A)
    outs = []
    for env in (BatchedTaskEnv(B, A, T, device=gpu_device).generate_instances(9),
                BatchedTaskEnv(B, A, T, device=gpu_device).load_instances(**inst)):
        outs.append(env.load_route_arrays(routes, lens).execute_routes())
    assert int(outs[1]["steps"].sum()) > B * T
    for k in outs[1]:
        assert torch.equal(outs[0][k], outs[1][k]) or (k == "summary" and np.array_equal(outs[0][k].cpu().numpy(), outs[1][k].cpu().numpy(),
                                                                                        equal_nan=True)), k


# ------------------------------------------------------------------ 4. raggedness switching on one handle
def test_uniform_ragged_uniform_on_one_handle(gpu_device, oracle_lib):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.graph_rollout import GraphedRollout
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    B, A, T = 48, 20, 50
    seeds = env_seeds(4, 0, B)
    inst = generate_batch(B, A, T, base_seed=21)
    env = BatchedTaskEnv(B, A, T, device=gpu_device).generate_instances(21)
    epoch = env.graph_epoch
    g = GraphedRollout(env, first_valid, check_every=4, record=True)
    summary, n = g.run(seeds)
    replay_recorded(oracle_lib, {k: v[:n] for k, v in g.rec.items()}, summary.cpu().numpy(), inst, seeds, A, T)
    graph_before = g.graph
    env.generate_instances(99)                                  # uniform again: the captured graph stays
    assert env.graph_epoch == epoch
    summary2, n2 = g.run(seeds)
    assert g.graph is graph_before
    replay_recorded(oracle_lib, {k: v[:n2] for k, v in g.rec.items()}, summary2.cpu().numpy(), generate_batch(B, A, T, base_seed=99), seeds, A, T)
    rag = generate_batch_ranges(range(700, 700 + B), (10, 20), (20, 50))
    env.generate_instances(700, (10, 20), (20, 50))             # ragged: per-env sizes pointer, other kernel instantiation
    assert env.graph_epoch == epoch + 1 and np.array_equal(env.n_tasks, rag["n_tasks"])
    summary3, n3 = g.run(seeds)
    assert g.graph is not graph_before
    replay_recorded(oracle_lib, {k: v[:n3] for k, v in g.rec.items()}, summary3.cpu().numpy(), rag, seeds, A, T,
                     n_agents=rag["n_agents"], n_tasks=rag["n_tasks"])
    env.generate_instances(21)                                  # ... and back
    assert env.graph_epoch == epoch + 2 and env.n_tasks is None
    summary4, _ = g.run(seeds)
    assert torch.equal(summary4, summary)
    # the host loaders and the generator switch each other's mode as well
    env.load_instances(**rag)
    assert env.graph_epoch == epoch + 3
    env.generate_instances(700, (10, 20), (20, 50))
    assert env.graph_epoch == epoch + 3
    summary5, _ = g.run(seeds)
    assert torch.equal(summary5, summary3)


# ------------------------------------------------------------------ 5. argument validation
def test_invalid_arguments_change_nothing(gpu_device):
    from dcmrta_amd import _lib
    from dcmrta_amd.batched_env import BatchedTaskEnv, DcmError
    from dcmrta_amd.choice import env_seeds
    B, A, T = 16, 20, 50
    env = BatchedTaskEnv(B, A, T, device=gpu_device, auto_reset=True, auto_reset_episodes=1).generate_instances(5)
    before = held_instances(env)
    obs = env.reset(env_seeds(3, 0, B))
    while bool(obs.active.any()):                               # eager auto-reset steps: terminal rows wait for the deferred flush
        obs = env.step(first_valid(obs).to(torch.int32))
    s = torch.arange(B, dtype=torch.int64, device=gpu_device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = lambda seeds, *a: env._lib.dcm_generate_instances(env._h, seeds, *a, stream)
    sp = C.c_void_p(s.data_ptr())
    for args in ((sp, 20, 21, 50, 50, 5, 5.0), (sp, 20, 20, 50, 51, 5, 5.0), (sp, 0, 20, 50, 50, 5, 5.0), (sp, 12, 11, 50, 50, 5, 5.0),
                 (sp, 20, 20, 0, 50, 5, 5.0), (sp, 20, 20, 50, 50, 0, 5.0), (sp, 20, 20, 50, 50, 6, 5.0), (None, 20, 20, 50, 50, 5, 5.0),
                 (sp, 20, 20, 50, 50, 5, -1.0), (sp, 20, 20, 50, 50, 5, float("nan"))):
        assert gen(*args) == -1, args                           # DCM_ERR_INVALID
        assert b"dcm_generate_instances" in env._lib.dcm_last_error()
    for kw in (dict(agents_range=(10, 21)), dict(tasks_range=51), dict(max_coalition_size=0), dict(max_coalition_size=6)):
        with pytest.raises(DcmError):
            env.generate_instances(5, **kw)
    assert env.n_tasks is None
    # the handle still holds its instances and its finished episodes' summaries
    assert_same_instances(held_instances(env), before)
    sm = env.summary().cpu().numpy()
    assert not np.isnan(sm).any()
    twin = BatchedTaskEnv(B, A, T, device=gpu_device, auto_reset=True, auto_reset_episodes=1).generate_instances(5)
    obs = twin.reset(env_seeds(3, 0, B))
    while bool(obs.active.any()):
        obs = twin.step(first_valid(obs).to(torch.int32))
    assert np.array_equal(sm, twin.summary().cpu().numpy())
    # a wide handle takes 16 and refuses 17
    wide = BatchedTaskEnv(4, A, T, device=gpu_device, member_cap=16)
    wide.generate_instances(0, max_coalition_size=16)
    with pytest.raises(DcmError):
        wide.generate_instances(0, max_coalition_size=17)
    d = torch.empty((1, 1), dtype=torch.float64, device=gpu_device)
    assert _lib.load().dcm_generator_draws(sp, 1, 1, 0, 0, C.c_void_p(d.data_ptr()), None, stream) == -1      # bound 0
    assert _lib.load().dcm_generator_draws(None, 1, 1, 5, 0, C.c_void_p(d.data_ptr()), None, stream) == -1
    fresh = BatchedTaskEnv(4, A, T, device=gpu_device)
    with pytest.raises(DcmError):
        fresh.instances()                                       # nothing loaded yet


# ------------------------------------------------------------------ 6. BatchedRunner(device_instances=True)
def _runner(gpu_device, device_instances, twin, use_graph):
    from dcmrta_amd.policy import AttentionNet
    from dcmrta_amd.runner import BatchedRunner
    torch.manual_seed(6)
    return BatchedRunner(n_envs=8, device=gpu_device, net_factory=lambda: AttentionNet(6, 5, 32), base_seed=21, twin_rollout=twin,
                         use_graph=use_graph, device_instances=device_instances)


@pytest.mark.parametrize("twin,use_graph", [(False, True), (True, True), (True, False)])
def test_runner_with_device_instances(gpu_device, twin, use_graph):
    """job() and testing() with the instances made on the device return what they return with the host generator: same weights,
    same torch RNG state, uniform and ragged calls."""
    out = []
    for device_instances in (False, True):
        r = _runner(gpu_device, device_instances, twin, use_graph)
        w = {k: v.clone() for k, v in r.get_weights().items()}
        res = {}
        for name, (an, tn) in (("uniform", (10, 20)), ("ragged", ((4, 9), (6, 15))), ("one_range", (7, (6, 15)))):
            torch.manual_seed(100)
            job, metrics, _ = r.job(w, w, 2, an, tn)
            res[name] = ([torch.stack(list(x)) if not isinstance(x, torch.Tensor) else x for x in job[:7]], metrics,
                         r.last["summary"].clone(), r.last["greedy_summary"].clone())
        res["testing_ragged"] = r.testing(seeds=range(30, 41))
        res["testing_uniform"] = r.testing(8, 12, seeds=[3, 2 ** 40 + 1, 5])
        res["testing_one"] = r.testing((4, 9), (6, 15), seed=77)
        out.append(res)
        r.close()
    host, dev = out
    for name in ("uniform", "ragged", "one_range"):
        for k in range(7):
            assert torch.equal(host[name][0][k], dev[name][0][k]), (name, k)
        assert host[name][0][0].shape[0] > 8
        assert host[name][1] == dev[name][1], name
        assert torch.equal(host[name][2], dev[name][2]) and torch.equal(host[name][3], dev[name][3]), name
    assert np.array_equal(host["testing_ragged"], dev["testing_ragged"]) and np.array_equal(host["testing_uniform"], dev["testing_uniform"])
    assert host["testing_one"] == dev["testing_one"]
