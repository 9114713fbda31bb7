"""CPU: the route-replay history golden (tests/golden/replay_history.npz, make_golden_replay_history.py) -- agent['route'] /
['arrival_time'], task['members'] / ['feasible_assignment'] and the generate_traj digests the reference leaves after
execute_by_route on the CTAS-D test set, static and reactive.

 * the oracle, the full-size yardstick of the GPU tests, reproduces the lists bit for bit;
 * trajectory.trajectories at max_waiting_time = 100 (what execute_by_route sets, env/task_env.py:564) reproduces every
   trajectory's sha256 and length."""
import hashlib
import os

import numpy as np
import pytest

from fixtures_ref import MODES, history


def test_fixture_covers_the_test_set(golden_dir):
    z = np.load(os.path.join(golden_dir, "replay_history.npz"))
    assert len(z["static_idx"]) >= 40 and len(z["reactive_idx"]) >= 30


@pytest.mark.parametrize("mode,reactive", MODES)
def test_oracle_replay_history_matches_reference(oracle_lib, golden_dir, mode, reactive):
    from dcmrta_amd.instances import load_instances_npz, load_routes_json
    inst, A = load_instances_npz(os.path.join(golden_dir, "instances_20A50T.npz"))
    routes = load_routes_json(os.path.join(golden_dir, "ctasd_routes.json"))
    for h in history(golden_dir, mode):
        i = h["i"]
        T = len(h["members"])
        o = oracle_lib.OracleEnv(A, T).load(inst["depot"][i], inst["task_xy"][i], inst["req"][i], inst["dur"][i])
        for a, r in enumerate(routes[i]):                                    # baselines/CTAS-D.py:41-45
            if r != [0]:
                o.pre_set_route(r[1:], a)
        fin = o.execute_by_route(reactive)
        for a in range(A):
            rt, ra = o.route(a)
            assert rt.tolist() == h["routes"][a][0] and ra.tolist() == h["routes"][a][1], (mode, i, a)
        for t in range(T):
            assert o.members(t).tolist() == h["members"][t], (mode, i, t)
        assert np.array_equal(fin["feasible"], h["feasible"]), (mode, i)


@pytest.mark.parametrize("mode,reactive", MODES)
def test_trajectories_at_mwt100_match_reference_digests(golden_dir, mode, reactive):
    from dcmrta_amd.instances import load_instances_npz
    from dcmrta_amd.trajectory import trajectories
    inst, _ = load_instances_npz(os.path.join(golden_dir, "instances_20A50T.npz"))
    for h in history(golden_dir, mode):
        i = h["i"]
        got = trajectories(h["routes"], inst["depot"][i], inst["task_xy"][i], h["members"], h["feasible"].astype(bool),
                           h["time_start"], h["time_finish"], h["current_time"], max_waiting_time=100.0)
        for a, g in enumerate(got):
            g = np.ascontiguousarray(g, np.float64)
            assert g.shape == (int(h["traj_len"][a]), 3), (mode, i, a, g.shape)
            assert hashlib.sha256(g.tobytes()).hexdigest() == h["traj_sha256"][a], (mode, i, a)
