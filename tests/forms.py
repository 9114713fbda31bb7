"""The machinery of the kernel-form tables (test infrastructure).  A test file keeps its own table

    id: (A, T, B, BatchedTaskEnv keywords, ragged ranges or None, scalar decision budget of a launch)

and its own base seeds in a Forms object; instances, the oracle's side of a launch and the handles come from here.  The oracle runs
are cached per module-level builder, keyed by the entry's values, so every file that uses the same entry shares them."""
import functools

import numpy as np

import oracle_ref as O


@functools.lru_cache(maxsize=None)
def _instances(A, T, B, ranges, uniform_base, ragged_base, choice_base, degen=False):
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    inst = generate_batch(B, A, T, base_seed=uniform_base + 3 * A + T) if ranges is None \
        else generate_batch_ranges(range(ragged_base, ragged_base + B), *ranges)
    return (degenerate(inst) if degen else inst), env_seeds(choice_base, 0, B)


def degenerate(inst):
    """A copy of a uniform generate_batch result with the edges an instance can have: task 2k+1 lies on task 2k (coincident pairs:
    `nearest` ties at equal rounded distance, agents on different tasks share a position in the group scan), tasks 0 and 1 lie on the
    depot (distance 0, travel time 0, arrival == now), and every third task has duration 0 (time_finish == time_start: it finishes in
    the event that starts it).  The requirements stay as generated."""
    out = {k: np.array(v, copy=True) for k, v in inst.items()}
    xy, T = out["task_xy"], out["task_xy"].shape[1]
    xy[:, 1:T:2] = xy[:, 0:T - 1:2]
    xy[:, 0] = xy[:, 1] = out["depot"]
    out["dur"][:, ::3] = 0.0
    return out


def _new_sims(A, T, B, mwt, ranges, bases, policy, max_time=100.0, degen=False):
    inst, seeds = _instances(A, T, B, ranges, *bases, degen)
    sims = []
    for b in range(B):
        a, t = (A, T) if ranges is None else (int(inst["n_agents"][b]), int(inst["n_tasks"][b]))
        sims.append(O.Sim(a, t, lambda j, one=O.one(inst, b, t): one, seeds[b], policy, mwt, max_time))
    return sims


@functools.lru_cache(maxsize=None)
def _sims(A, T, B, mwt, ranges, budget, bases, policy, episodes, max_time=100.0, degen=False):
    sims = _new_sims(A, T, B, mwt, ranges, bases, policy, max_time, degen)
    return sims, np.array([s.launch(episodes, budget) for s in sims], np.int64)


class Forms:
    def __init__(self, forms, big_forms, uniform_base, ragged_base, choice_base, degenerate=()):
        """degenerate: the ids of the forms that play degenerate() of their generated instances"""
        self.all, self.big, self.bases = {**forms, **big_forms}, big_forms, (uniform_base, ragged_base, choice_base)
        self.degenerate = frozenset(degenerate)

    def instances(self, form):
        """(instances, choice seeds) of a form: computed once, shared, never changed."""
        A, T, B, _, ranges, _ = self.all[form]
        return _instances(A, T, B, ranges, *self.bases, form in self.degenerate)

    def sims(self, form, policy, episodes):
        """The oracle's side of one launch of `episodes` episodes on a form under its budget, (Sim per env, steps per env): computed
        once, shared, never changed."""
        A, T, B, kw, ranges, budget = self.all[form]
        return _sims(A, T, B, kw.get("max_waiting_time", 10.0), ranges, budget, self.bases, policy, episodes, kw.get("max_time", 100.0), form in self.degenerate)

    def episodes(self, form, policy, episodes):
        """The oracle's episodes 0 .. episodes-1 of every env of a form, one per unlimited launch: [b][k] = an object with .o and .a."""
        A, T, B, kw, ranges, _ = self.all[form]
        out = []
        for s in _new_sims(A, T, B, kw.get("max_waiting_time", 10.0), ranges, self.bases, policy, kw.get("max_time", 100.0), form in self.degenerate):
            eps = []
            for _ in range(episodes):
                s.launch(1, -1)
                assert s.done
                eps.append(type("Episode", (), dict(o=s.o, a=s.a))())
            out.append(eps)
        return out

    def env(self, gpu_device, form):
        """(a handle with the form's instances loaded, not reset; the choice seeds)."""
        from dcmrta_amd.batched_env import BatchedTaskEnv
        A, T, B, kw, _, _ = self.all[form]
        inst, seeds = self.instances(form)
        env = BatchedTaskEnv(B, A, T, device=gpu_device, **kw).load_instances(**inst)
        assert (env.record_bytes() > 65536) == (form in self.big)
        return env, seeds


def snap(env, steps):
    """Everything a launch leaves: steps, records, summary rows, the return log (env._ring), status, episode counts, the observation
    buffers and -- if it is set -- the rollout log.  As bytes."""
    o = env.obs()
    st = env.status()
    parts = dict(steps=steps, state=env.clone_state(), summary=env.summary(), ring=env._ring, flags=st["flags"], decisions=st["decisions"],
                 now=st["now"], episodes=env.episodes(), agents=o.agents, tasks=o.tasks, mask=o.mask)
    if getattr(env, "_rollout_route", None) is not None:
        parts.update(zip(("log_task", "log_arrival", "log_len"), env.rollout_routes()))
    return {k: np.ascontiguousarray((v if isinstance(v, np.ndarray) else v.cpu().numpy())).copy() for k, v in parts.items()}


def assert_same(got, ref, tag):
    assert sorted(got) == sorted(ref), tag
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), f"{tag}: {k}"
