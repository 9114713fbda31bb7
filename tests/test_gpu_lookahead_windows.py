"""-m gpu: the device lookahead policy (k_la_rollout_random / k_larn_rollout_random, csrc/rollout_lookahead.hpp) on every Sim<>
instantiation of its form and through every branch of its restore: a window of K lookahead decisions deep inside an episode
(lookahead_policy_ref.WINDOWS), where agents have been abandoned more than sixteen times, members wait on tasks and the env's state
is anything but fresh.  The only kernel that rewinds an env must put it back exactly: a wrong restore plays on from a slightly wrong
state and still ends in a plausible plan.

Per case three yardsticks, all bit for bit and for EVERY env of the batch (a wrong slice pitch shows in a neighbour):
  1. the oracle walker stopped behind the window (lookahead_window): steps, decision counter, member lists, abandonment counts, task
     and agent state, clock, and the rollout log;
  2. a second handle that takes the same window on the host -- Lookahead.values() -> best_actions -> step, K times: the bytes of
     clone_state() (records, summary rows, abandonment rows AND overflow count tables) and of status().  A count table that was not
     zeroed, or not copied back, differs here.  (Uniform cases; Lookahead refuses a ragged batch.);
  3. after the window the base policy plays the episode to its end: summary row, flags and log against window_tail's oracle
     episode.  What a restore left wrong and only matters later shows here.
tests/test_lookahead_window_ref_host.py proves from the oracle alone what each case meets.  The renewing form runs at 50A/200T (MG)
with its window across the end of the first episode."""
import time

import numpy as np
import pytest

import lookahead_policy_ref as LP
import oracle_ref as O

pytestmark = pytest.mark.gpu

CAP = 64
TASK_KEYS = ("n_members", "n_abandoned", "feasible", "finished", "time_start", "time_finish")


def handle(gpu_device, name, inst):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    c = LP.WINDOWS[name]
    env = BatchedTaskEnv(c["B"], c["A"], c["T"], device=gpu_device, max_waiting_time=c["mwt"], **c.get("kw", {})).load_instances(**inst)
    return env.enable_rollout_log(CAP)


def prefix(env, seeds, policy, d0):
    """reset and the ordinary form up to the window; none at all where every window starts at decision 0, so that the lookahead launch
    is the handle's first launch"""
    env.reset(seeds, observe=False)
    if d0.any():
        steps = env.rollout(policy, episodes=1, write_obs=False, max_decisions=d0).cpu().numpy()
        assert np.array_equal(steps, d0), (steps, d0)


def getters(env):
    ag, st = env.agents_state(), env.status()
    return dict(mem=env.task_members().cpu().numpy(), abc=env.abandoned_counts().cpu().numpy(),
                ts={k: v.cpu().numpy() for k, v in env.tasks_state().items()},
                ag={k: ag[k].cpu().numpy() for k in ("sum_waiting_time", "travel_dist", "returned")},
                st={k: v.cpu().numpy() for k, v in st.items()})


def assert_stopped(tag, got, b, a, t, s, member_cap):
    """env b of a handle against the oracle walker where the window ended (LP.stopped_state)"""
    st, mem, abc = got["st"], got["mem"][b], got["abc"][b]
    assert int(st["decisions"][b]) == s["decisions"] and not (st["flags"][b] & LP.DONE), (tag, "decisions / flags", st["decisions"][b], st["flags"][b])
    assert st["now"][b] == s["now"], (tag, "now", st["now"][b], s["now"])
    want = np.full((t, member_cap), -1, np.int16)
    for j, m in enumerate(s["members"]):
        want[j, :len(m)] = m
    assert np.array_equal(mem[:t], want), (tag, "members", np.flatnonzero((mem[:t] != want).any(1)))
    assert (mem[t:] == -1).all(), (tag, "members beyond the env's tasks")
    assert np.array_equal(abc[:a, :t], s["abc"]), (tag, "abandonment counts", np.argwhere(abc[:a, :t] != s["abc"])[:8])
    assert not abc[a:].any() and not abc[:, t:].any(), (tag, "abandonment counts beyond the env's sizes")
    for k in TASK_KEYS:
        v = got["ts"][k][b, :t].astype(s["tasks"][k].dtype)
        assert np.array_equal(v, s["tasks"][k]), (tag, k, np.flatnonzero(v != s["tasks"][k]))
    for k, v in (("agent_wait", got["ag"]["sum_waiting_time"][b, :a]), ("travel_dist", got["ag"]["travel_dist"][b, :a]),
                 ("returned", got["ag"]["returned"][b, :a]), ("task_wait", got["ts"]["sum_waiting_time"][b, :t])):
        assert np.array_equal(v.astype(s[k].dtype), s[k]), (tag, k, np.flatnonzero(v.astype(s[k].dtype) != s[k]))


@pytest.mark.parametrize("name", list(LP.WINDOWS))
def test_a_window_of_lookahead_decisions(gpu_device, oracle_lib, name):
    import torch
    from dcmrta_amd.lookahead import Lookahead
    c = LP.WINDOWS[name]
    inst, seeds, sz = LP.window_instances(name)
    ws = LP.windows(name)
    B, K, policy = c["B"], c["K"], c["policy"]
    member_cap = c.get("kw", {}).get("member_cap", 5)
    d0 = np.array([x["d0"] for x in ws], np.int64)

    dev = handle(gpu_device, name, inst)
    prefix(dev, seeds, policy, d0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = dev.rollout(policy, episodes=1, write_obs=False, lookahead=True, max_decisions=K).cpu().numpy()
    print(f"{name}: {LP.window_sim_kind(name)} B={B} K={K} lookahead launch {time.perf_counter() - t0:.3f} s")

    # 1. against the oracle walker stopped at d0 + K
    assert np.array_equal(steps, np.full(B, K)), (name, steps)
    got, log = getters(dev), O.log(dev)
    for b, (a, t) in enumerate(sz):
        assert_stopped(f"{name} env {b}", got, b, a, t, ws[b]["stop"], member_cap)
        O.assert_log(log, b, LP.Stopped(ws[b]["stop"], a), f"{name} window")

    # 2. against the same window taken on the host
    if not c.get("sizes"):
        host = handle(gpu_device, name, inst)
        prefix(host, seeds, policy, d0)
        la = Lookahead(host, policy)
        for i in range(K):
            reward, finished = la.values()
            host.step(la.best_actions(reward, finished), observe=False)
        assert dev.clone_state().cpu().numpy().tobytes() == host.clone_state().cpu().numpy().tobytes(), (name, "clone_state")
        hs = host.status()
        for k, v in dev.status().items():
            assert v.cpu().numpy().tobytes() == hs[k].cpu().numpy().tobytes(), (name, "status", k)
        la.close(); host.close()

    # 3. the base policy plays on to the end of the episode
    more = dev.rollout(policy, episodes=1, write_obs=False).cpu().numpy()
    sm, st, log = dev.summary().cpu().numpy(), {k: v.cpu().numpy() for k, v in dev.status().items()}, O.log(dev)
    for b, x in enumerate(ws):
        tail, tag = x["tail"], f"{name} tail env {b}"
        assert int(more[b]) == tail["n_steps"] - x["d0"] - K and int(st["decisions"][b]) == tail["n_steps"], (tag, more[b], st["decisions"][b], tail["n_steps"])
        O.assert_summary(sm[b], tail["result"], tag)
        assert int(st["flags"][b]) == tail["flags"], (tag, st["flags"][b], tail["flags"])
        O.assert_log(log, b, LP.Episode(tail), tag)
    assert (dev.episodes().cpu().numpy() == 1).all()
    dev.close()


def test_the_renewing_form_at_an_mg_shape(gpu_device, oracle_lib):
    """k_larn_rollout_random<50,200,false>: prefix to two decisions in front of the end of episode 1, then one launch of two episodes
    whose budget puts exactly one decision behind the restart.  Episode 1's end: the non-renewing handle (and the oracle).  The decision
    behind the restart -- all 200 tasks unmasked, a snapshot per inner episode on the fresh instance: a fresh handle on the next
    instances under the shifted seed, one values() + step on the host."""
    import torch
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.lookahead import Lookahead
    c = LP.RENEWING
    A, T, B, policy = c["A"], c["T"], c["B"], c["policy"]
    inst_seeds, seeds, ws = LP.renewing_windows()
    d0, end, K = (np.array([x[k] for x in ws], np.int64) for k in ("d0", "end", "K"))

    def gen(s, renew):
        env = BatchedTaskEnv(B, A, T, device=gpu_device, max_waiting_time=c["mwt"])
        env.generate_instances(s)
        if renew:
            env.set_instance_renewal(c["stride"])
        env.enable_rollout_log(CAP)
        env.enable_return_log(2)
        return env

    renewing = gen(inst_seeds, True)
    prefix(renewing, seeds, policy, d0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = renewing.rollout(policy, episodes=2, write_obs=False, lookahead=True, max_decisions=K).cpu().numpy()
    print(f"renewing 50A/200T: launch {time.perf_counter() - t0:.3f} s")
    assert np.array_equal(steps, K), (steps, K)
    assert (renewing.instance_index().cpu().numpy() == 1).all() and (renewing.episodes().cpu().numpy() == 1).all()
    st = {k: v.cpu().numpy() for k, v in renewing.status().items()}
    assert np.array_equal(st["decisions"], end + 1) and not (st["flags"] & LP.DONE).any()

    # episode 1: the non-renewing handle plays the same window to the episode's end
    first = gen(inst_seeds, False)
    prefix(first, seeds, policy, d0)
    n1 = first.rollout(policy, episodes=1, write_obs=False, lookahead=True).cpu().numpy()
    assert np.array_equal(n1, end - d0), (n1, end, d0)
    ring, sm = renewing._retlog.cpu().numpy(), first.summary().cpu().numpy()
    assert renewing.summary().cpu().numpy().tobytes() == sm.tobytes()           # the row is episode 1's until episode 2 ends
    for b, x in enumerate(ws):
        O.assert_summary(sm[b], x["result"], f"renewing env {b}: episode 1")
        assert ring[b, 0] == x["result"]["reward"] and np.isnan(ring[b, 1]), (b, ring[b])

    # the decision behind the restart
    second = gen(inst_seeds + np.uint64(c["stride"]), False)
    second.reset(np.array([LP.shifted_seed(seeds[b], end[b]) for b in range(B)], np.uint64), observe=False)
    la = Lookahead(second, policy)
    reward, finished = la.values()
    second.step(la.best_actions(reward, finished), observe=False)
    got, want = getters(renewing), getters(second)
    assert got["st"]["now"].tobytes() == want["st"]["now"].tobytes()
    for k in ("mem", "abc"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for part in ("ts", "ag"):
        for k in want[part]:
            assert got[part][k].tobytes() == want[part][k].tobytes(), (part, k)
    la.close(); renewing.close(); first.close(); second.close()
