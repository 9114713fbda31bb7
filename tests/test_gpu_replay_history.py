"""-m gpu: the route-replay log (dcm_set_replay_log) -- agent['route'] / ['arrival_time'], task['members'] /
['feasible_assignment'] after execute_by_route (env/task_env.py:562-593), what generate_traj reads (:375-418).

 * reference known answer (tests/golden/replay_history.npz): both kernels, static and reactive, + the trajectory digests
 * the TaskEnv facade after the baselines/CTAS-D.py:59-94 loop
 * BASELINE config-5 size (100A/500T) against the oracle; the log leaves every other output byte-identical
 * edges: a short log, a second replay, the log switched off, a too narrow member table, the lockstep log untouched"""
import copy
import hashlib
import os

import numpy as np
import pytest
import torch

from fixtures_ref import MODES, history

pytestmark = pytest.mark.gpu
KEYS_EXACT = ("finished", "time_start", "time_finish", "task_wait", "n_members", "travel_dist", "returned", "agent_wait")


def _ctasd_batch(golden_dir):
    from dcmrta_amd.instances import load_instances_npz, load_routes_json
    inst, A = load_instances_npz(os.path.join(golden_dir, "instances_20A50T.npz"))
    routes = load_routes_json(os.path.join(golden_dir, "ctasd_routes.json"))
    rl = [[(None if r == [0] else r[1:]) for r in routes[i]] + [None] * (A - len(routes[i])) for i in range(50)]
    return inst, A, routes, rl


def _digests(trajs):
    return [(len(t), hashlib.sha256(np.ascontiguousarray(t, np.float64).tobytes()).hexdigest()) for t in trajs]


def _check_against_history(out, b, h, name):
    A = len(h["routes"])
    n = out["route_len"][b].cpu().numpy()
    rt, ra = out["route"][b].cpu().numpy(), out["arrival"][b].cpu().numpy()
    for a in range(A):
        assert n[a] == len(h["routes"][a][0]), (name, a)
        assert rt[a, :n[a]].tolist() == h["routes"][a][0] and ra[a, :n[a]].tolist() == h["routes"][a][1], (name, a)
    mem = out["members"][b].cpu().numpy()
    for t, m in enumerate(h["members"]):
        assert mem[t, :len(m)].tolist() == m and (mem[t, len(m):] == -1).all(), (name, t)
    assert np.array_equal(out["feasible"][b].cpu().numpy(), h["feasible"]), name
    assert int(n.sum()) == int(out["steps"][b]), name


@pytest.mark.parametrize("mode,reactive", MODES)
# auto + member_cap 8: the register-resident kernel for these shapes; lds / hbm: the general kernel with its scratch there
@pytest.mark.parametrize("placement,cap", [("auto", 8), ("lds", 8), ("lds", 16), ("hbm", 8), ("hbm", 16)])
def test_replay_log_reference_known_answer(gpu_device, golden_dir, mode, reactive, placement, cap):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.trajectory import replay_trajectories
    inst, A, _, rl = _ctasd_batch(golden_dir)
    env = BatchedTaskEnv(50, A, 50, device=gpu_device)
    env.load_instances(**inst)
    env.load_routes(rl, member_cap=cap)
    env.set_replay_placement(placement)
    env.enable_replay_log(cap=64)
    out = env.execute_routes(reactive=reactive)
    flags = out["flags"].cpu().numpy()
    hs = history(golden_dir, mode)
    assert len(hs) >= (40 if mode == "static" else 30)
    for h in hs:
        i = h["i"]
        name = f"{mode} {placement} cap={cap} instance {i}"
        assert not (flags[i] & 0x78), name
        _check_against_history(out, i, h, name)
        assert _digests(replay_trajectories(env, out, i)) == list(zip(h["traj_len"].tolist(), h["traj_sha256"].tolist())), name
    env.close()


def test_facade_dicts_after_ctasd_loop(gpu_device, golden_dir):
    """baselines/CTAS-D.py:59-94 on the facade (as test_ctasd_baseline_loop_on_facade): agent_dic / task_dic then carry the
    reference's route, arrival, member and feasibility lists, and generate_traj from those dicts matches the reference's."""
    from dcmrta_amd.task_env import TaskEnv
    from dcmrta_amd.trajectory import trajectories
    inst, A, routes, _ = _ctasd_batch(golden_dir)
    hs = {h["i"]: h for h in history(golden_dir, "static")}
    for i in (0, 7, 23):
        env = TaskEnv.from_arrays(A, inst["depot"][i], inst["task_xy"][i], inst["req"][i], inst["dur"][i], device=gpu_device)
        env.reactive_planning = False
        env.clear_decisions()
        for a, r in enumerate(routes[i]):                                    # CTAS-D.py:41-45
            if r == [0]:
                continue
            env.pre_set_route(copy.copy(r)[1:], a)
        env.force_wait = True
        env.execute_by_route("./", "CTAS-D", False)                          # :77
        env.get_episode_reward(100)
        h = hs[i]
        ad, td = env.agent_dic, env.task_dic
        for a in range(A):
            assert ad[a]["route"] == h["routes"][a][0] and ad[a]["arrival_time"] == h["routes"][a][1], (i, a)
        for t in range(50):
            assert td[t]["members"] == h["members"][t], (i, t)
            assert td[t]["feasible_assignment"] == bool(h["feasible"][t]), (i, t)
        got = trajectories([(ad[a]["route"], ad[a]["arrival_time"]) for a in range(A)], env.depot["location"],
                           np.stack([td[t]["location"] for t in range(50)]), [td[t]["members"] for t in range(50)],
                           np.array([td[t]["feasible_assignment"] for t in range(50)]),
                           np.array([td[t]["time_start"] for t in range(50)]), np.array([td[t]["time_finish"] for t in range(50)]),
                           env.current_time, max_waiting_time=env.max_waiting_time)
        assert _digests(got) == list(zip(h["traj_len"].tolist(), h["traj_sha256"].tolist())), i


# ---------------------------------------------------------------------------------------------------- BASELINE config-5 size
B5, A5, T5, CAP5 = 256, 100, 500, 256


@pytest.fixture(scope="module")
def config5_batch(oracle_lib):
    """100A/500T, synthetic routes (as bench.py --config 5), each env replayed once in the oracle per mode: padded oracle
    route / arrival / length / member / feasibility arrays."""
    from dcmrta_amd.instances import generate_batch, synthetic_routes
    inst = generate_batch(B5, A5, T5, base_seed=4242)
    out = {}
    for mode, reactive in MODES:
        rl = [synthetic_routes(inst["req"][b], A5, max_task=100 if reactive else None) for b in range(B5)]
        ref = dict(route=np.full((B5, A5, CAP5), -2, np.int16), arrival=np.zeros((B5, A5, CAP5)), route_len=np.zeros((B5, A5), np.int32),
                   members=np.full((B5, T5, 8), -1, np.int16), feasible=np.zeros((B5, T5), np.uint8), truncated=np.zeros(B5, bool))
        for b in range(B5):
            o = oracle_lib.OracleEnv(A5, T5).load(inst["depot"][b], inst["task_xy"][b], inst["req"][b], inst["dur"][b])
            for a, r in enumerate(rl[b]):
                o.pre_set_route(r, a)
            fin = o.execute_by_route(reactive)
            ref["truncated"][b] = bool(fin["truncated"])
            ref["feasible"][b] = fin["feasible"]
            for a in range(A5):
                rt, ra = o.route(a)
                assert len(rt) <= CAP5
                ref["route_len"][b, a] = len(rt)
                ref["route"][b, a, :len(rt)] = rt
                ref["arrival"][b, a, :len(rt)] = ra
            for t in range(T5):
                m = o.members(t)
                assert len(m) <= 5
                ref["members"][b, t, :len(m)] = m
        out[mode] = (rl, ref)
    return inst, out


def _run5(gpu_device, inst, rl, reactive, cap, placement, log):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    env = BatchedTaskEnv(B5, A5, T5, device=gpu_device)
    env.load_instances(**inst)
    env.load_routes(rl, member_cap=cap)
    env.set_replay_placement(placement)
    if log:
        env.enable_replay_log(cap=CAP5)
    out = {k: v.clone() for k, v in env.execute_routes(reactive=reactive).items()}
    env.close()
    return out


@pytest.mark.parametrize("mode,reactive", MODES)
@pytest.mark.parametrize("cap", [5, 8])
def test_replay_log_matches_oracle_at_config5_size(gpu_device, config5_batch, mode, reactive, cap):
    """Static replays have 500 live tasks: the general kernel (auto's choice too); reactive ones at the reference's cap of 100: the
    register-resident kernel under auto.  Reactive at T = 500 ends TRUNCATED in both (test_replay_matches_oracle): compared too.
    The same batch without the log gives byte-identical steps, flags, per-task / per-agent outputs and summary rows."""
    inst, per_mode = config5_batch
    rl, ref = per_mode[mode]
    for placement in ("auto", "lds", "hbm"):
        name = f"{mode} cap={cap} {placement}"
        out = _run5(gpu_device, inst, rl, reactive, cap, placement, True)
        flags = out["flags"].cpu().numpy()
        assert ((flags & 4) != 0).tolist() == ref["truncated"].tolist() and not (flags & 0x78).any(), name
        assert ref["truncated"].all() == reactive, name
        n = out["route_len"].cpu().numpy()
        assert np.array_equal(n, ref["route_len"]), name
        assert np.array_equal(n.sum(1), out["steps"].cpu().numpy()), name             # one entry per agent_step
        valid = np.arange(CAP5)[None, None, :] < n[:, :, None]
        assert np.array_equal(np.where(valid, out["route"].cpu().numpy(), -2), ref["route"]), name
        assert np.array_equal(np.where(valid, out["arrival"].cpu().numpy(), 0.0).view(np.uint64), ref["arrival"].view(np.uint64)), name
        mem = out["members"].cpu().numpy()
        assert mem.shape == (B5, T5, cap) and np.array_equal(mem, ref["members"][:, :, :cap]), name
        assert np.array_equal(out["feasible"].cpu().numpy(), ref["feasible"]), name
        plain = _run5(gpu_device, inst, rl, reactive, cap, placement, False)
        for k in ("steps", "flags", "summary") + KEYS_EXACT:
            a, b = out[k], plain[k]
            assert torch.equal(a.view(torch.uint8) if a.dtype.is_floating_point else a,
                               b.view(torch.uint8) if b.dtype.is_floating_point else b), (name, k)
        assert not {"route", "members"} & set(plain), name


# ---------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("placement", ["auto", "hbm"])
def test_replay_log_edges(gpu_device, golden_dir, placement):
    from dcmrta_amd import _lib
    from dcmrta_amd.batched_env import BatchedTaskEnv
    inst, A, _, rl = _ctasd_batch(golden_dir)
    hs = history(golden_dir, "static")
    env = BatchedTaskEnv(50, A, 50, device=gpu_device)
    env.load_instances(**inst)
    env.load_routes(rl, member_cap=8)
    env.set_replay_placement(placement)
    # a lockstep route log on the same handle: a replay does not write it
    lock = env.enable_route_log(cap=16).routes()
    # cap = 2: the stored prefix is right and route_len counts every entry
    env.enable_replay_log(cap=2)
    out = env.execute_routes()
    for h in hs:
        i = h["i"]
        n = out["route_len"][i].cpu().numpy()
        rt, ra = out["route"][i].cpu().numpy(), out["arrival"][i].cpu().numpy()
        for a, (r, arr) in enumerate(h["routes"]):
            assert n[a] == len(r) and rt[a, :min(2, len(r))].tolist() == r[:2] and ra[a, :min(2, len(r))].tolist() == arr[:2], (i, a)
    assert (lock[0] == -2).all() and (lock[1] == 0).all() and (lock[2] == 0).all()
    # a second execute_routes restarts the log
    env.enable_replay_log(cap=64)
    out = env.execute_routes()
    first = {k: out[k].clone() for k in ("route", "arrival", "route_len", "members", "feasible")}
    out = env.execute_routes()
    for k, v in first.items():
        assert torch.equal(out[k], v), k
    for h in hs:
        _check_against_history(out, h["i"], h, f"second replay {h['i']}")
    # all NULL disables: the buffers are untouched by a replay
    bufs = {k: out[k] for k in first}
    for v in bufs.values():
        v.fill_(7)
    env.enable_replay_log(0)
    out2 = env.execute_routes()
    torch.cuda.synchronize()
    assert "route" not in out2 and all(bool((v == 7).all()) for v in bufs.values())
    # member_cols < member_cap: refused before anything is launched
    env.enable_replay_log(cap=64)
    r = env._rlog
    for v in r.values():
        v.fill_(7)
    sm = env.summary().clone()
    _lib.check(env._lib.dcm_set_replay_log(env._h, r["route"].data_ptr(), r["arrival"].data_ptr(), r["route_len"].data_ptr(), 64,
                                      r["members"].data_ptr(), 5, r["feasible"].data_ptr()))
    with pytest.raises(_lib.DcmError):
        env.execute_routes()
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in r.values()) and torch.equal(env.summary().view(torch.uint8), sm.view(torch.uint8))
    assert (lock[2] == 0).all()
    env.close()
