"""Instance and size renewal against the oracle (test infrastructure): episode k of an env plays the host generator's instance of
seed renewal_seeds(seed, k, stride) -- with its own sizes where a range is a (lo, hi) tuple; an int range is the fixed size -- under the
decision counter that runs on across the episodes.  An instance is the pair (A_k, instance dict) in both cases."""
import functools

import numpy as np

import helpers as H
import oracle_ref as O

M64 = 1 << 64
EPISODES = 3


def dim(r):
    return int(r[1]) if isinstance(r, tuple) else int(r)


def inst_seeds(base, B):
    return np.array([(base + b) % M64 for b in range(B)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def host_instance(ar, tr, seed, mcs):
    from dcmrta_amd.instances import generate_instance_ranges
    return generate_instance_ranges(ar, tr, int(seed), max_coalition_size=mcs)


@functools.lru_cache(maxsize=None)
def oracle_chain(ar, tr, inst_seed, stride, choice_seed, mcs=5, n=EPISODES, indices=None, policy="random", mwt=10.0, max_time=100.0):
    """Episodes 0..n-1 of one env under renewal: (rollout results, (A_k, instance) per episode), computed once per env and shared.
    indices: episode k plays the instance of index indices[k] instead of k (an env whose renewal was turned off on the way)."""
    from dcmrta_amd.instances import renewal_seeds
    insts = [host_instance(ar, tr, int(renewal_seeds(inst_seed, k, stride)), mcs) for k in (range(n) if indices is None else indices)]
    eps = [dict(n_steps=r["n_steps"], row=O.summary_row(r)) for r in O.episodes(None, None, insts.__getitem__, choice_seed, policy, len(insts), mwt, max_time=max_time)]
    return eps, insts


def chains(ar, tr, B, base, stride, choice_seeds, mcs=5, rows=None):
    return {b: oracle_chain(ar, tr, (base + b) % M64, stride, int(choice_seeds[b]), mcs) for b in (range(B) if rows is None else rows)}


def make(gpu_device, B, ar, tr, base, stride, mcs=5, member_cap=5, **kw):
    """A handle at the ranges' maxima (flagged to renew sizes where there is a range) with generated instances base + 0..B-1, renewal
    on, a return log of EPISODES columns; not reset yet."""
    from dcmrta_amd.batched_env import BatchedTaskEnv
    if isinstance(ar, tuple) or isinstance(tr, tuple):
        kw = dict(renew_sizes=True, **kw)
    env = BatchedTaskEnv(B, dim(ar), dim(tr), device=gpu_device, member_cap=member_cap, **kw)
    env.generate_instances(inst_seeds(base, B), agents_range=ar, tasks_range=tr, max_coalition_size=mcs)
    env.set_instance_renewal(stride)
    return env, env.enable_return_log(EPISODES)


def held(env):
    return {k: v.cpu().numpy() for k, v in env.instances().items() if v is not None}


def assert_instance(held, b, sized_inst):
    """Env b holds this (A, instance), padded as instances.generate_batch_ranges pads (xy 0, req 1, dur 0 beyond the env's T).  On a
    uniform batch instances() returns no size arrays and there is no padding."""
    A, inst = sized_inst
    t = inst["req"].shape[0]
    if "n_agents" in held:
        assert held["n_agents"][b] == A and held["n_tasks"][b] == t, (b, held["n_agents"][b], held["n_tasks"][b], A, t)
    assert np.array_equal(held["depot"][b], inst["depot"]), b
    assert np.array_equal(held["task_xy"][b, :t], inst["task_xy"]) and not held["task_xy"][b, t:].any(), b
    assert np.array_equal(held["req"][b, :t], inst["req"]) and (held["req"][b, t:] == 1).all(), b
    assert np.array_equal(held["dur"][b, :t], inst["dur"]) and not held["dur"][b, t:].any(), b


def assert_after(env, ring, chains, steps=None, rows=None):
    """What every path must leave after EPISODES episodes in the envs `rows` (default: all): the returns, the last episode's summary
    row, the last index, the last instance with its sizes, the decision count."""
    rows = range(env.B) if rows is None else rows
    sm, rl, idx, hd = env.summary().cpu().numpy(), ring.cpu().numpy(), env.instance_index().cpu().numpy(), held(env)
    assert np.array_equal(env.episodes().cpu().numpy()[rows], np.full(len(rows), EPISODES))
    for b in rows:
        eps, insts = chains[b]
        assert np.array_equal(rl[b], np.array([e["row"][0] for e in eps])), b
        assert np.array_equal(sm[b], eps[-1]["row"], equal_nan=True), b
        assert idx[b] == EPISODES - 1, (b, idx[b])
        assert_instance(hd, b, insts[-1])
        if steps is not None:
            assert steps[b] == sum(e["n_steps"] for e in eps), b


def lockstep_to_end(env, seeds, read_summary_every=0, policy=None):
    """Step an auto-resetting handle until every env is inactive; actions from the choice protocol's host mirror."""
    B = env.B
    obs = env.reset(seeds)
    dcount = np.zeros(B, np.int64)
    for s in range(4001):
        active = obs.active.cpu().numpy()
        if not active.any():
            break
        assert s < 4000, "envs still active after 4000 steps"
        if policy is None:
            mk = obs.mask.cpu().numpy().astype(np.uint8)
            act = np.array([H.host_random_action(mk[b], int(seeds[b]), int(dcount[b])) if active[b] else 0 for b in range(B)], np.int32)
        else:
            act = policy(obs)
        obs = env.step(act)
        dcount += active
        if read_summary_every and s % read_summary_every == read_summary_every - 1:
            env.summary()                       # completes the deferred rows on the way
    return dcount


def first_valid(obs):
    import torch
    return torch.argmax((~obs.mask).to(torch.int32), dim=1)   # lowest unmasked action id
