"""Member removal against the oracle (test infrastructure): one episode walked through the oracle's step-wise API, which shows the
member lists in front of and behind every task_update call, and what the removals of a batch cover."""
import numpy as np

import helpers as H

MAX_TIME = 100.0


def walk_episode(o, req, seed_e):
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
    while not finished and o.now < MAX_TIME:                               # worker.py:45
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
