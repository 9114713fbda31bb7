"""bench.py's line layout (CPU): the summary object is last, compact, and auxiliary failures are found; --dump-outputs writes the
last timed pass in env order, a fixed sample of it beyond the size limit."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _line():
    big = {"workload": "x" * 3000}
    return {"metric": "env_steps_per_sec", "value": 1.4e9, "unit": "steps/s", "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 1.05,
            "ms_per_step_min": 1.01, "ms_per_step_max": 1.2, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "roofline": {"kernel": "k_rollout_fast", "frac": 0.5234567, "frac_hi": 0.6, "salu_issue_frac": 0.4, "stale": False, "bulk": "y" * 500},
            "parity": {"envs_checked": 4096, "mismatches": 0, "fields": ["a"] * 20},
            "config": dict(big),
            "lockstep_kernel": {"envs": 65536, "frac": 0.75, "traffic_frac": 0.57, "rocprof_avg_launch_us": 143.7, "steady_state_us": 16.5},
            "other_configs": {"config4_shard": {"value": 8.1e8, "roofline": {"frac": 0.45}, "parity": {"envs_checked": 8192, "mismatches": 0},
                                                "cpu_baseline": {"value": 1e7}, "workload": "w" * 2000},
                              "config3": {"value": 5e6}},
            "cpu_baseline": {"value": 1.7e7, "cores": 16, "sample": "s" * 400}}


def test_summary_is_last_and_fits_the_tail():
    import bench
    out = bench.order_line(_line())
    keys = list(out)
    assert keys[-4:] == ["roofline", "parity", "cpu_baseline", "summary"]
    assert keys.index("config") < keys.index("roofline") and keys.index("other_configs") < keys.index("roofline")
    assert keys[:3] == ["metric", "value", "unit"]
    s = json.dumps(out)
    tail = s[-2000:]
    sm = json.dumps(out["summary"])
    assert len(sm) < 1500 and tail.endswith(sm + "}")
    assert out["summary"]["roofline"]["frac"] == 0.5235 and out["summary"]["parity"] == {"envs_checked": 4096, "mismatches": 0}
    assert out["summary"]["config4_shard"] == {"value": 8.1e8, "frac": 0.45, "parity_mismatches": 0, "parity_envs": 8192, "cpu": 1e7}
    assert out["summary"]["lockstep_kernel"]["steady_state_us"] == 16.5


def test_auxiliary_failures_are_reported():
    import bench
    j = _line()
    assert bench.aux_failures(j) == []
    j["other_configs"]["config4_shard"]["parity"]["mismatches"] = 3
    j["other_configs"]["config3"] = {"error": "RuntimeError: boom"}
    j["lockstep_kernel"] = {"error": "x"}
    bad = bench.aux_failures(j)
    assert len(bad) == 3 and any("3 of 8192" in b for b in bad) and any("boom" in b for b in bad)


def _fake_subs(sizes, A=3, T=4, EP=2, replay=False):
    """Stand-ins of bench.SubBatch after a timed pass (CPU tensors): what dump_outputs reads from them."""
    import types

    import torch
    subs = []
    for k, B in enumerate(sizes):
        g = torch.Generator().manual_seed(k)
        env = types.SimpleNamespace(device=torch.device("cpu"))
        sm = torch.rand((B, 8), dtype=torch.float64, generator=g)
        ob = types.SimpleNamespace(agents=torch.rand((B, A, 6), generator=g), tasks=torch.rand((B, T + 1, 5), generator=g),
                                   mask=torch.rand((B, T + 1), generator=g) < 0.5)
        env.summary, env.obs = (lambda sm=sm: sm), (lambda ob=ob: ob)
        steps = torch.randint(50, 200, (B,), dtype=torch.int64, generator=g)
        sb = types.SimpleNamespace(B=B, replay=replay, env=env, counts=[steps + 1, steps],
                                   ring=torch.rand((B, EP), dtype=torch.float64, generator=g))
        sb.last_out = {"steps": steps, "flags": torch.zeros((B,), dtype=torch.int32), "summary": sm}
        subs.append(sb)
    return subs


def _load(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_the_last_pass_in_env_order(tmp_path):
    import numpy as np
    import bench
    subs = _fake_subs([5, 7])
    bench.dump_outputs(subs, str(tmp_path / "a"), 100, True)
    d = _load(tmp_path / "a")
    assert sorted(d) == ["env_index", "obs_agents", "obs_mask", "obs_tasks", "returns", "steps", "summary"]
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    assert d["obs_agents"].dtype == np.float32 and d["steps"].dtype == np.float64
    np.testing.assert_array_equal(d["env_index"], np.arange(100, 112))
    np.testing.assert_array_equal(d["steps"], np.concatenate([sb.counts[-1].numpy() for sb in subs]))
    np.testing.assert_array_equal(d["returns"], np.concatenate([sb.ring.numpy() for sb in subs]))
    np.testing.assert_array_equal(d["obs_mask"], np.concatenate([sb.env.obs().mask.numpy() for sb in subs]).astype(np.float32))
    assert d["obs_tasks"].shape == (12, 5, 5) and d["summary"].shape == (12, 8)
    bench.dump_outputs(_fake_subs([5, 7]), str(tmp_path / "b"), 100, False)
    assert sorted(_load(tmp_path / "b")) == ["env_index", "returns", "steps", "summary"]


def test_dump_outputs_samples_large_batches_the_same_way_every_time(tmp_path):
    import numpy as np
    import bench
    limit = 40 * 1024
    for name in ("a", "b"):
        bench.dump_outputs(_fake_subs([300, 200]), str(tmp_path / name), 0, True, limit=limit)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= limit
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    idx = a["env_index"].astype(np.int64)
    assert 0 < len(idx) < 500 and np.all(np.diff(idx) > 0)
    full = np.concatenate([sb.ring.numpy() for sb in _fake_subs([300, 200])])
    np.testing.assert_array_equal(a["returns"], full[idx])


def test_dump_outputs_of_the_route_replay(tmp_path):
    import numpy as np
    import bench
    subs = _fake_subs([4, 4], replay=True)
    bench.dump_outputs(subs, str(tmp_path), 8, True, suffix=".rank1")
    d = _load(tmp_path)
    assert sorted(d) == ["env_index.rank1", "flags.rank1", "steps.rank1", "summary.rank1"]
    np.testing.assert_array_equal(d["steps.rank1"], np.concatenate([sb.last_out["steps"].numpy() for sb in subs]))
