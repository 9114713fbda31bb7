"""Member removal against the oracle (test infrastructure): one episode walked through the oracle's step-wise API, which shows the
member lists in front of and behind every task_update call, what the removals of a batch cover, and a handle against the walk's
snapshot in front of a decision (assert_state, assert_obs; assert_handover: both, the header fields and the agent side)."""
import numpy as np

import helpers as H
import oracle_ref as O

MAX_TIME = 100.0
TASK_KEYS = ("n_members", "n_abandoned", "feasible", "finished", "time_start", "time_finish")


def walk_episode(o, req, seed_e, max_time=MAX_TIME):
    """One episode of the oracle through its step-wise API (the loop of worker.py:45-87 restated).  Returns (snaps, removals): the
    state in front of every decision, and one entry (task, rule, members before, positions that left) per task and task_update call
    that removed somebody."""
    from dcmrta_amd.choice import below, draw
    A, T = o.A, o.T
    members = [np.zeros(0, np.int32) for _ in range(T)]
    ab = np.zeros((A, T), np.int32)
    nab = np.zeros(T, np.int32)
    removals, snaps = [], []
    state = {}

    def task_update():
        o.task_update()
        f = o.final()
        for t in np.flatnonzero(f["n_abandoned"] != nab):
            old, new = members[t], o.members(t)
            left = [j for j, a in enumerate(old) if a not in new]
            assert len(left) == f["n_abandoned"][t] - nab[t] and len(new) == len(old) - len(left)
            removals.append((int(t), "spread" if req[t] - len(old) <= 0 else "wait", old.copy(), left))      # env/task_env.py:254
            for j in left:
                ab[old[j], t] += 1
            members[t] = new
        nab[:] = f["n_abandoned"]
        state.update(f)

    finished, d, empty = False, 0, 0
    while not finished and o.now < max_time:                               # worker.py:45
        ids, t = o.next_decision()                                         # :47
        groups = o.get_unique_group(ids) if len(ids) else []              # :48
        o.now = t                                                          # :49
        task_update()                                                      # :50
        o.agent_update()                                                   # :51
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
                snaps.append(dict(leader=leader, now=o.now, mask=mask, agents_obs=ag, tasks_obs=tk,
                                  members=list(members), abandoned=ab.copy(),       # (the arrays are replaced, never written)
                                  **{k: state[k] for k in ("n_members", "n_abandoned", "feasible", "finished", "time_start", "time_finish")}))
                action = H.host_random_action(mask, seed_e, d)
                snaps[-1]["action"] = action
                vacancy = int(tk[action, 0]) if action >= 1 else len(group)            # :327 (the status may be stale)
                group.remove(leader)                                       # :328
                step = [leader]
                if vacancy > 1:                                            # :330-333
                    for j in range(min(vacancy - 1, len(group))):
                        step.append(group.pop(below(draw(seed_e, d, 2 + j), len(group))))
                for m in step:
                    o.agent_step(m, action)                                # :338-340
                if action >= 1:
                    members[action - 1] = o.members(action - 1)
                task_update()                                              # :74
                o.agent_update()                                           # :76
                d += 1
        finished = o.check_finished()                                      # :85
    return snaps, removals


def coverage(rem):
    """what the removals of a batch (per env: walk_episode's list) show"""
    slots5, wait_skip, spread_multi, two_tasks = set(), 0, 0, 0
    for env_rem in rem:
        by_agent = {}
        for t, rule, old, left in env_rem:
            if len(old) == 5:
                slots5.update(left)
            if rule == "wait" and any(q - p >= 2 for p, q in zip(left, left[1:])):
                wait_skip += 1
            if rule == "spread" and len(left) >= 2:
                spread_multi += 1
            for j in left:
                by_agent.setdefault(int(old[j]), set()).add(t)
        two_tasks += sum(1 for ts in by_agent.values() if len(ts) >= 2)
    return dict(slots5=slots5, wait_skip=wait_skip, spread_multi=spread_multi, two_tasks=two_tasks,
                calls=sum(len(r) for r in rem))


class Lists:
    """The member lists of one env's snapshots as a -1 padded table, kept up to date from snapshot to snapshot: walk_episode
    replaces a list's array when the list changes and never writes to one, so only rows whose array is another one are redone."""

    def __init__(self, T, cap):
        self.table, self.seen = np.full((T, cap), -1, np.int16), [None] * T

    def at(self, members):
        for t, m in enumerate(members):
            if m is not self.seen[t]:
                self.table[t] = -1
                self.table[t, :len(m)] = m
                self.seen[t] = m
        return self.table


def assert_state(tag, s, lists, a, t, mem, abc, ts):
    """the state of one env (rows of the getters) against the snapshot in front of a decision; rows beyond the env's own sizes are empty"""
    want = lists.at(s["members"])
    assert np.array_equal(mem[:t], want), (tag, "members", np.flatnonzero((mem[:t] != want).any(1)))
    assert np.all(mem[t:] == -1), (tag, "members beyond T_e")
    ab = np.zeros(abc.shape, np.int16)
    idx, val = s["abandoned"]
    ab[idx // t, idx % t] = val
    assert np.array_equal(abc, ab), (tag, "abandonment counts", np.argwhere(abc != ab)[:8])
    for k in TASK_KEYS:
        assert np.array_equal(ts[k][:t].astype(s[k].dtype), s[k]), (tag, k, np.flatnonzero(ts[k][:t].astype(s[k].dtype) != s[k]))


def assert_obs(tag, s, a, t, ag, tk, mk):
    assert np.array_equal(mk[:t + 1].astype(np.uint8), s["mask"]) and np.all(mk[t + 1:] == 1), (tag, "mask")
    assert np.array_equal(ag[:a], s["agents_obs"]) and np.all(ag[a:] == -1.0), (tag, "agents observation")
    assert np.array_equal(tk[:t + 1], s["tasks_obs"]) and np.all(tk[t + 1:] == -1.0), (tag, "tasks observation")




def sparse_abandoned(snaps):
    """Replace every snapshot's dense abandonment table by (flat indices, values) of its non-zero entries: what assert_state takes."""
    for x in snaps:
        ab = x.pop("abandoned")
        idx = np.flatnonzero(ab)
        x["abandoned"] = (idx, ab.ravel()[idx].astype(np.int16))
    return snaps


def read_batch(env, obs=None):
    """A batch's getters, read once: task_members, abandoned_counts, tasks_state, agents_state, status and observe() -- or, in place of
    observe(), the Observation `obs` that the step() call just made returned."""
    o = env.observe() if obs is None else obs
    ag = env.agents_state()
    return dict(mem=env.task_members().cpu().numpy(), abc=env.abandoned_counts().cpu().numpy(),
                ts={k: v.cpu().numpy() for k, v in env.tasks_state().items()},
                ag={k: ag[k].cpu().numpy() for k in ("sum_waiting_time", "travel_dist", "returned")},
                st={k: v.cpu().numpy() for k, v in env.status().items()},
                obs=tuple(x.cpu().numpy() for x in (o.agents, o.tasks, o.mask, o.leader, o.active)))


def assert_handover(tag, got, b, d, snaps, lists, a, t, inst_one, seed, mwt, max_time=MAX_TIME):
    """Env b of a handle (got: read_batch) against the walk's snapshot in front of decision d (snaps: the env's list; d == len(snaps): the
    episode is over): leader, now, the decision counter and the active bit; assert_state, with nothing in the rows beyond the env's own
    sizes; assert_obs; and the agent side against the oracle's own episode stopped in front of that decision."""
    ag, tk, mk, ld, act = got["obs"]
    st, abc = got["st"], got["abc"][b]
    assert st["decisions"][b] == d, (tag, "decision counter", int(st["decisions"][b]), d)
    if d >= len(snaps):
        assert not act[b] and (st["flags"][b] & 1), (tag, "the episode must be over")
    else:
        s = snaps[d]
        assert act[b] and not (st["flags"][b] & 1), (tag, "the episode must not be over")
        assert int(ld[b]) == s["leader"] and st["now"][b] == s["now"], (tag, "leader / now", int(ld[b]), s["leader"], st["now"][b], s["now"])
        assert_state(tag, s, lists, a, t, got["mem"][b], abc[:a, :t], {k: v[b] for k, v in got["ts"].items()})
        assert not abc[a:].any() and not abc[:, t:].any(), (tag, "abandonment counts beyond the env's sizes")
        assert_obs(tag, s, a, t, ag[b], tk[b], mk[b])
    # dcm_get_agents / dcm_get_tasks compute the waiting sums on read, at the state the env is in; the oracle computes them when an episode
    # ends (env/task_env.py:344-364, :421), so an episode that the cap stopped is given that one call here -- it changes nothing else
    o, _, ended = O.play(a, t, inst_one, seed, 0, "random", d, mwt, max_time)
    if not ended:
        import oracle
        oracle.lib().orc_finish_episode(o._h)
    fin = o.final()
    for k, v in (("agent_wait", got["ag"]["sum_waiting_time"][b, :a]), ("travel_dist", got["ag"]["travel_dist"][b, :a]),
                 ("returned", got["ag"]["returned"][b, :a]), ("task_wait", got["ts"]["sum_waiting_time"][b, :t])):
        assert np.array_equal(v.astype(fin[k].dtype), fin[k]), (tag, k, np.flatnonzero(v.astype(fin[k].dtype) != fin[k]))
