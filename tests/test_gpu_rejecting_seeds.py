"""-m gpu: the on-device instance generator where a bounded draw is REJECTED (csrc/instgen.hpp, wave_bounded).  The wave takes 128
words per block by jump-ahead on the assumption that Lemire's method rejects none; when one is rejected it falls back to the
sequential routine from the start of that block, with the stream state -- has_uint32, uinteger, the 128-bit state -- that the blocks
before it left behind.  At max_coalition_size <= 16 a word is rejected with probability <= 9 / 2^32, so ordinary seeds never get there:

  1. dcm_generator_draws at bounds that reject a word in 512 / in 128: the fall-back starts in every block, after 0..7 full ones;
  2. dcm_generate_instances on the seeds of tests/golden/rejecting_seeds.json (tests/test_rejecting_seeds_host.py proves with numpy
     that each of them rejects where recorded), and the buffered half-word carried across blocks on ordinary seeds;
  3. the same seeds as the instance an env RENEWS to inside every kernel form that compiles the renewal separately.

Every comparison is exact: numpy itself for 1, the host generators of dcmrta_amd/instances.py for 2, the oracle on host-generated
instances for 3 (the chains of renewal_ref.py, as in test_gpu_instance_renewal / test_gpu_size_renewal)."""
import functools
import os

import numpy as np
import pytest
import torch

import renewal_ref as R
from fixtures_ref import BIG_SEEDS, assert_same_instances, held_instances, load_rejecting_seeds, no_rejection_form, numpy_words
from renewal_ref import EPISODES, M64

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the stream at a bound that rejects now and then
def _draw_seeds(n):
    return np.concatenate([np.arange(n - len(BIG_SEEDS), dtype=np.uint64), np.array(BIG_SEEDS, dtype=np.uint64)])


def _rejected_words(seed, nd, bound, n):
    """Indices (in stream order) of the rejected words among those n values of integers(0, bound) consume after nd doubles: from
    numpy's raw draws, Lemire's acceptance evaluated on the host."""
    g = np.random.default_rng(int(seed))
    g.random(nd)
    raw = g.bit_generator.random_raw(n)                                  # 2 n words: enough for n values at these bounds
    words = np.stack([raw & np.uint64(0xFFFFFFFF), raw >> np.uint64(32)], axis=1).reshape(-1)
    rej = np.flatnonzero(((words * np.uint64(bound)) & np.uint64(0xFFFFFFFF)) < np.uint64(((1 << 32) - bound) % bound))
    k = 0                                                                # the n values consume n + (rejected words among them) words
    while k < len(rej) and rej[k] < n + k:
        k += 1
    assert n + k <= len(words)
    return rej[:k]


@functools.lru_cache(maxsize=None)
def rejection_coverage(nd, bound, n, n_seeds):
    """(seeds per first-rejecting block, seeds without a rejection, seeds with two or more, set of first rejected words)."""
    blocks, none, twice, firsts = np.zeros((n + 127) // 128, np.int64), 0, 0, set()
    for s in _draw_seeds(n_seeds):
        rej = _rejected_words(s, nd, bound, n)
        if len(rej) == 0:
            none += 1
            continue
        blocks[rej[0] // 128] += 1
        twice += len(rej) >= 2
        firsts.add(int(rej[0]))
    return blocks, none, twice, firsts


# bound (threshold 2^32 mod bound = 2^23: a word in 512; 2^25: a word in 128), number of integers, number of seeds -- the smallest
# power of two at which numpy alone meets the coverage asserted below, with n_doubles 0 and with 3
DRAW_CASES = [pytest.param(2 ** 31 - 2 ** 22, 1024, 8192, id="1-in-512-eight-blocks"),
              pytest.param(2 ** 31 - 2 ** 24, 300, 2048, id="1-in-128-short-last-block")]


@pytest.mark.parametrize("nd", [0, 3])
@pytest.mark.parametrize("bound,n,n_seeds", DRAW_CASES)
def test_generator_draws_with_occasional_rejections(gpu_device, bound, n, n_seeds, nd):
    from dcmrta_amd.batched_env import device_generator_draws
    blocks, none, twice, firsts = rejection_coverage(nd, bound, n, n_seeds)
    print("seeds per first-rejecting block %s, none %d, twice or more %d" % (blocks.tolist(), none, twice))
    assert (blocks > 0).all() and none > 0 and twice > 0, (blocks, none, twice)
    assert {0, 127, 128, n - 1} <= firsts, sorted(firsts)
    seeds = _draw_seeds(n_seeds)
    d, i = device_generator_draws(seeds, nd, bound, n, device=gpu_device)
    assert d.shape == (n_seeds, nd) and i.shape == (n_seeds, n)
    for k, s in enumerate(seeds):
        g = np.random.default_rng(int(s))
        assert np.array_equal(d[k], g.random(nd)), (bound, nd, s)
        assert np.array_equal(i[k], g.integers(0, bound, n).astype(np.uint32)), (bound, nd, s)


# ------------------------------------------------------------------ 2. dcm_generate_instances on the fixture seeds
@pytest.fixture(scope="module")
def fixture_seeds(golden_dir):
    return load_rejecting_seeds(golden_dir)


def _rejects(e):
    """The guard of every case below: the instance of fixture entry e is NOT what a generator that never rejects would make."""
    from dcmrta_amd.instances import generate_instance_ranges
    ar, tr, m = e["agents_range"], e["tasks_range"], e["max_coalition_size"]
    A, inst = generate_instance_ranges(ar, tr, e["seed"], max_coalition_size=m)
    _, T, _, words = numpy_words(e["seed"], ar, tr, m)
    w = e["first_rejected_word"]
    closed = no_rejection_form(words, T, m)
    assert (A, T) == (e["A"], e["T"]) and np.array_equal(inst["req"][:w], closed[:w]) and inst["req"][w] != closed[w], e["seed"]
    assert not np.array_equal(inst["req"][w:], closed[w:])
    return A, inst


# one case per class the fixture holds (NEEDED in test_rejecting_seeds_host.py says which it must hold)
CLASSES = sorted(load_rejecting_seeds(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")))


@pytest.mark.parametrize("name", CLASSES)
def test_generate_instances_on_rejecting_seeds(gpu_device, fixture_seeds, name):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.instances import generate_batch_ranges
    entries = fixture_seeds[name]
    for e in entries:
        _rejects(e)
    ar, tr, m = entries[0]["agents_range"], entries[0]["tasks_range"], entries[0]["max_coalition_size"]
    A, T = R.dim(ar), R.dim(tr)
    B = 32
    fx = [e["seed"] for e in entries]
    # fixture seeds between ordinary ones, at both ends of the batch and in the middle
    seeds = np.array(fx[:1] + list(range(900, 900 + B - len(fx) - len(BIG_SEEDS))) + fx[1:-1] + BIG_SEEDS + fx[-1:] if len(fx) > 1
                     else list(range(900, 900 + B - 1 - len(BIG_SEEDS))) + fx + BIG_SEEDS, dtype=np.uint64)
    assert len(seeds) == B
    want = generate_batch_ranges([int(s) for s in seeds], ar, tr, max_coalition_size=m)
    ragged = isinstance(ar, tuple) or isinstance(tr, tuple)
    if not ragged:
        want["n_agents"] = want["n_tasks"] = None
    env = BatchedTaskEnv(B, A, T, device=gpu_device, member_cap=16 if m > 5 else 5)
    env.generate_instances(seeds, ar, tr, max_coalition_size=m)
    assert_same_instances(held_instances(env), want, name)
    env.generate_instances(0)                                            # other instances in between
    env.generate_instances(torch.from_numpy(seeds.view(np.int64)).to(gpu_device), ar, tr, m)
    assert_same_instances(held_instances(env), want, name)
    if ragged:
        assert np.array_equal(env.n_agents, want["n_agents"]) and np.array_equal(env.n_tasks, want["n_tasks"])


@pytest.mark.parametrize("m", [3, 5])
@pytest.mark.parametrize("ranges", [((50, 100), 300), (100, (130, 500)), ((3, 128), 1023)])
def test_buffered_half_word_across_blocks(gpu_device, ranges, m):
    """One size drawn and more than 128 tasks: lane 0 of every block after the first takes the high half lane 63 left behind.
    Ordinary seeds, no rejection."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.instances import generate_batch_ranges
    ar, tr = ranges
    B = 128
    seeds = np.array(list(range(600, 600 + B - len(BIG_SEEDS))) + BIG_SEEDS, dtype=np.uint64)
    want = generate_batch_ranges([int(s) for s in seeds], ar, tr, max_coalition_size=m)
    assert want["n_tasks"].max() > 128
    env = BatchedTaskEnv(B, R.dim(ar), R.dim(tr), device=gpu_device).generate_instances(seeds, ar, tr, max_coalition_size=m)
    assert np.array_equal(env.n_agents, want["n_agents"]) and np.array_equal(env.n_tasks, want["n_tasks"])
    assert_same_instances(held_instances(env), want, (ranges, m))
    env.generate_instances(torch.from_numpy(seeds.view(np.int64)).to(gpu_device), ar, tr, m)
    assert_same_instances(held_instances(env), want, (ranges, m))


# ------------------------------------------------------------------ 3. the fall-back inside the kernels that restart episodes
def _renewing_batch(entries, B, stride, base):
    """Instance seeds of a batch whose env b renews INTO fixture seed S_b at its restart k_b (1 and 2 in turn), i.e. starts from
    S_b - k_b * stride mod 2^64; the envs between them start from ordinary seeds.  Returns (seeds, {env: (k, entry)})."""
    seeds = [(base + b) % M64 for b in range(B)]
    at = {}
    for j, e in enumerate(entries):
        b = (j * (B - 1)) // max(1, len(entries) - 1) if len(entries) > 1 else B // 2     # spread over the batch, both ends
        k = 1 + j % 2
        seeds[b] = (e["seed"] - k * stride) % M64
        at[b] = (k, e)
    assert len(at) == len(entries) < B and {k for k, _ in at.values()} == {1, 2}
    return seeds, at


def _make(gpu_device, B, A, T, inst_seeds, stride, mcs, member_cap=5, ar=None, tr=None, **kw):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    env = BatchedTaskEnv(B, A, T, device=gpu_device, member_cap=member_cap, **kw)
    env.generate_instances(np.array(inst_seeds, dtype=np.uint64), ar, tr, max_coalition_size=mcs)
    env.set_instance_renewal(stride)
    return env, env.enable_return_log(EPISODES)


def _uniform_case(fixture_seeds, name, B, choice_base):
    """(A, T, mcs, instance seeds, stride, choice seeds, oracle chains) of a uniform batch that renews into the class's seeds, after
    the guards: episode k_b of env b IS the fixture instance, and that instance rejects."""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import renewal_seeds
    entries = fixture_seeds[name][:3]
    A, T, mcs = entries[0]["A"], entries[0]["T"], entries[0]["max_coalition_size"]
    stride = B
    inst_seeds, at = _renewing_batch(entries, B, stride, 7000)
    seeds = env_seeds(choice_base, 0, B)
    chains = {b: R.oracle_chain(A, T, inst_seeds[b], stride, int(seeds[b]), mcs) for b in range(B)}
    for b, (k, e) in at.items():
        assert int(renewal_seeds(inst_seeds[b], k, stride)) == e["seed"]
        _, inst = _rejects(e)
        assert np.array_equal(chains[b][1][k][1]["req"], inst["req"]) and np.array_equal(chains[b][1][k][1]["task_xy"], inst["task_xy"])
    return A, T, mcs, inst_seeds, stride, seeds, chains


# fixture class, batch, member_cap: one case per form of dcm_rollout_random that compiles the renewal separately
ROLLOUT_CASES = [
    pytest.param("m5_20A50T", 8, 5, id="20A50T-k_rn_rollout_fast"),
    pytest.param("m5_50A200T_later_block", 8, 5, id="50A200T-k_rn_rollout_fast_mc-second-block"),
    pytest.param("m5_70A130T", 8, 5, id="70A130T-k_rn_rollout_fast_g"),
    pytest.param("m5_100A500T_third_block_on", 4, 5, id="100A500T-k_rn_rollout_random"),
    pytest.param("m13_20A50T", 8, 16, id="20A50T-wide-13"),
]


@pytest.mark.parametrize("name,B,member_cap", ROLLOUT_CASES)
def test_persistent_rollout_renews_into_a_rejecting_seed(gpu_device, fixture_seeds, name, B, member_cap):
    A, T, mcs, inst_seeds, stride, seeds, chains = _uniform_case(fixture_seeds, name, B, 71)
    env, ring = _make(gpu_device, B, A, T, inst_seeds, stride, mcs, member_cap)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=EPISODES).cpu().numpy()
    R.assert_after(env, ring, chains, steps)


@pytest.mark.parametrize("route_log", [pytest.param(False, id="k_rn_step_fast"), pytest.param(True, id="route-log-k_rn_step")])
def test_lockstep_auto_reset_renews_into_a_rejecting_seed(gpu_device, fixture_seeds, route_log):
    B = 8
    A, T, mcs, inst_seeds, stride, seeds, chains = _uniform_case(fixture_seeds, "m5_20A50T", B, 73)
    env, ring = _make(gpu_device, B, A, T, inst_seeds, stride, mcs, auto_reset=True, auto_reset_episodes=EPISODES)
    if route_log:
        env.enable_route_log()
    dcount = R.lockstep_to_end(env, seeds, 40)
    R.assert_after(env, ring, chains, dcount)
    assert np.array_equal(env.status()["decisions"].cpu().numpy(), dcount)


def _sized_case(fixture_seeds, B, choice_base):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import renewal_seeds
    entries = fixture_seeds["m5_both_ranged"][:4]
    ar, tr, mcs = entries[0]["agents_range"], entries[0]["tasks_range"], entries[0]["max_coalition_size"]
    stride = B
    inst_seeds, at = _renewing_batch(entries, B, stride, 17000)
    seeds = env_seeds(choice_base, 0, B)
    chains = {b: R.oracle_chain(ar, tr, inst_seeds[b], stride, int(seeds[b]), mcs) for b in range(B)}
    for b, (k, e) in at.items():
        assert int(renewal_seeds(inst_seeds[b], k, stride)) == e["seed"]
        A, inst = _rejects(e)
        cA, cinst = chains[b][1][k]
        assert (cA, cinst["req"].shape[0]) == (e["A"], e["T"]) and np.array_equal(cinst["req"], inst["req"])
    return ar, tr, mcs, inst_seeds, stride, seeds, chains, at


def _assert_fixture_sizes(env, at):
    """The fixture seed also fixes the env's sizes: an env whose LAST restart drew it holds the fixture's A and T."""
    held = R.held(env)
    last = [(b, e) for b, (k, e) in at.items() if k == EPISODES - 1]
    assert last
    for b, e in last:
        assert (held["n_agents"][b], held["n_tasks"][b]) == (e["A"], e["T"]), b


def test_size_renewing_rollout_renews_into_a_rejecting_seed(gpu_device, fixture_seeds):
    B = 8
    ar, tr, mcs, inst_seeds, stride, seeds, chains, at = _sized_case(fixture_seeds, B, 75)
    env, ring = _make(gpu_device, B, R.dim(ar), R.dim(tr), inst_seeds, stride, mcs, ar=ar, tr=tr, renew_sizes=True)
    env.reset(seeds, observe=False)
    steps = env.rollout_random(episodes=EPISODES).cpu().numpy()
    R.assert_after(env, ring, chains, steps)
    _assert_fixture_sizes(env, at)


def test_size_renewing_lockstep_renews_into_a_rejecting_seed(gpu_device, fixture_seeds):
    B = 8
    ar, tr, mcs, inst_seeds, stride, seeds, chains, at = _sized_case(fixture_seeds, B, 77)
    env, ring = _make(gpu_device, B, R.dim(ar), R.dim(tr), inst_seeds, stride, mcs, ar=ar, tr=tr, renew_sizes=True,
                      auto_reset=True, auto_reset_episodes=EPISODES)
    dcount = R.lockstep_to_end(env, seeds, 40)
    R.assert_after(env, ring, chains, dcount)
    _assert_fixture_sizes(env, at)
    assert np.array_equal(env.status()["decisions"].cpu().numpy(), dcount)
