"""Readers of the golden fixtures and small host mirrors that more than one test file uses (test infrastructure)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- trajectories and replays
def traj_fixture(golden_dir, name):
    """A traj_*.npz of the reference: (the arrays, (route, arrival times) per agent, member lists, trajectories per agent)."""
    z = np.load(os.path.join(golden_dir, name))
    A = z["route"].shape[0]
    routes = []
    for a in range(A):
        n = int((z["route"][a] != -2).sum())
        routes.append(([int(x) for x in z["route"][a, :n]], [float(x) for x in z["arrival"][a, :n]]))
    members = [[int(x) for x in row if x >= 0] for row in z["members"]]
    ends = np.cumsum(z["traj_len"])
    ref = [z["traj"][e - n:e] for e, n in zip(ends, z["traj_len"])]
    return z, routes, members, ref


def extra_instance(meta):
    """Instance of an entry of trace_hashes_extra.json (tests/golden/make_golden_extra.py)."""
    from dcmrta_amd.instances import generate_instance, generate_instance_ranges
    if meta["kind"] == "ranges":
        A, inst = generate_instance_ranges((10, 20), (20, 50), meta["inst_seed"])
    elif meta["kind"] == "arrays":           # hand-modified instance (coincident locations): arrays stored with the digest
        A = meta["A"]
        inst = dict(depot=np.array(meta["depot"]), task_xy=np.array(meta["task_xy"]), req=np.array(meta["req"], np.int32),
                    dur=np.array(meta["dur"]))
    else:
        A = meta["A"]
        inst = generate_instance(A, meta["T"], meta["inst_seed"], meta.get("max_coalition_size", 5), meta.get("max_duration", 5.0))
    assert (A, len(inst["req"])) == (meta["A"], meta["T"])
    assert int(inst["req"].sum()) == meta["req_sum"] and float(inst["dur"][0]) == meta["dur0"]
    return A, inst


def random_replay_cases(golden_dir):
    """tests/golden/replay_random.json: (case, instance dict) pairs; instances from the test set or the seeded generator."""
    from dcmrta_amd.instances import generate_instance, load_instances_npz
    cases = json.load(open(os.path.join(golden_dir, "replay_random.json")))
    ts, _ = load_instances_npz(os.path.join(golden_dir, "instances_20A50T.npz"))
    out = []
    for c in cases:
        if c["kind"] == "testset":
            inst = {k: ts[k][c["index"]] for k in ("depot", "task_xy", "req", "dur")}
        else:
            inst = generate_instance(c["A"], c["T"], c["inst_seed"])
        assert int(inst["req"].sum()) == c["req_sum"]
        out.append((c, inst))
    return out


def schedule_cases(golden_dir):
    """tests/golden/replay_schedule.json (make_golden_schedule.py): replays of the reference with its four dynamic-arrival
    constants substituted (env/task_env.py:567, :221) -> (case, instance dict) pairs."""
    from dcmrta_amd.instances import generate_instance
    out = []
    for c in json.load(open(os.path.join(golden_dir, "replay_schedule.json"))):
        inst = generate_instance(c["A"], c["T"], c["inst_seed"])
        assert int(inst["req"].sum()) == c["req_sum"]
        out.append((c, inst))
    return out


MODES = [("static", False), ("reactive", True)]


def history(golden_dir, mode):
    """tests/golden/replay_history.npz, per fixture instance of the mode: (instance, routes, members, feasible, time_start,
    time_finish, current_time, traj_len, traj_sha256)."""
    z = np.load(os.path.join(golden_dir, "replay_history.npz"))
    out = []
    for k, i in enumerate(z[f"{mode}_idx"].tolist()):
        n = z[f"{mode}_route_len"][k]
        routes = [([int(x) for x in z[f"{mode}_route"][k, a, :n[a]]], [float(x) for x in z[f"{mode}_arrival"][k, a, :n[a]]])
                  for a in range(len(n))]
        members = [[int(x) for x in row if x >= 0] for row in z[f"{mode}_members"][k]]
        out.append(dict(i=i, routes=routes, members=members, feasible=z[f"{mode}_feasible"][k],
                        time_start=z[f"{mode}_time_start"][k], time_finish=z[f"{mode}_time_finish"][k],
                        current_time=float(z[f"{mode}_current_time"][k]), traj_len=z[f"{mode}_traj_len"][k],
                        traj_sha256=z[f"{mode}_traj_sha256"][k]))
    return out


def replay_recorded(oracle_lib, rec, summary, inst, seeds, A, T, n_agents=None, n_tasks=None):
    """Every episode of a recorded batched rollout ([S, B, ...] experience + `active`) through the oracle with the recorded
    actions injected: leaders, observations, masks, reward and metrics must be the reference env's."""
    act = rec["active"].cpu().numpy()
    ag, tk, mk, ac, ld = (rec[k].cpu().numpy() for k in ("agents", "tasks", "mask", "action", "leader"))
    summary = np.asarray(summary)
    for b in range(act.shape[1]):
        a = int(n_agents[b]) if n_agents is not None else A
        t = int(n_tasks[b]) if n_tasks is not None else T
        sel = act[:, b]
        o = oracle_lib.OracleEnv(a, t).load(inst["depot"][b], inst["task_xy"][b, :t], inst["req"][b, :t], inst["dur"][b, :t])
        ref = o.rollout(int(seeds[b]), 0, oracle_lib.POLICY_INJECTED, cap_steps=8192, inj_action=ac[sel, b].astype(np.int32))
        assert ref["n_steps"] == int(sel.sum()), b
        assert np.array_equal(ref["leader"], ld[sel, b]), b
        assert np.array_equal(ref["agents_obs"], ag[sel, b, :a]) and np.array_equal(ref["tasks_obs"], tk[sel, b, :t + 1]), b
        assert np.array_equal(ref["mask"], mk[sel, b, :t + 1].astype(np.uint8)), b
        assert ref["reward"] == summary[b, 0], b
        for i in range(6):
            assert ref["metrics"][i] == summary[b, 2 + i], (b, i)


def anymask_action(mask_row, seed_e, d, T):
    """Host mirror of ORC_POLICY_ANY / tests/golden/make_golden_masked.py: a policy that does not respect the mask."""
    from dcmrta_amd.choice import below, draw
    r = draw(seed_e, d, 1)
    if r % 16 == 1:
        return 0
    if r % 4 == 0:
        return 1 + (r >> 4) % T
    valid = np.flatnonzero(mask_row == 0)
    return int(valid[below(r, len(valid))])


# ---------------------------------------------------------------------------------------------------- generated instances
BIG_SEEDS = [2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 17, 2 ** 63, 2 ** 63 + 2 ** 31 + 5, 12345678901234567890, 2 ** 64 - 1]


def held_instances(env):
    """What the handle holds, on the host; the size arrays are None on a uniform batch."""
    return {k: (None if v is None else v.cpu().numpy()) for k, v in env.instances().items()}


def assert_same_instances(got, want, what=""):
    for k in ("depot", "task_xy", "req", "dur"):
        assert got[k].dtype == np.asarray(want[k]).dtype and np.array_equal(got[k], want[k]), (what, k)
    for k in ("n_agents", "n_tasks"):
        if want.get(k) is None:
            assert got[k] is None, (what, k)
        else:
            assert np.array_equal(got[k], want[k]), (what, k)


# ---------------------------------------------------------------------------------------------------- rejecting seeds
def load_rejecting_seeds(golden_dir):
    """tests/golden/rejecting_seeds.json as {class: [entry, ...]} with the ranges as generate_instances takes them: an int, or a
    (lo, hi) tuple."""
    tup = lambda r: tuple(r) if isinstance(r, list) else r
    with open(os.path.join(golden_dir, "rejecting_seeds.json")) as f:
        classes = json.load(f)["classes"]
    return {name: [dict(e, agents_range=tup(e["agents_range"]), tasks_range=tup(e["tasks_range"])) for e in entries]
            for name, entries in classes.items()}


def numpy_words(seed, agents_range, tasks_range, m):
    """np.random.default_rng(seed) up to the requirements: the sizes, random(2 + A + 2 T), then has_uint32 / uinteger of the bit
    generator's state and its raw draws as 32-bit words in stream order, the buffered half first when there is one.
    Returns A, T, has, words (at least 2 T of them)."""
    g = np.random.default_rng(int(seed))
    T = int(g.integers(tasks_range[0], tasks_range[1] + 1)) if isinstance(tasks_range, tuple) else int(tasks_range)
    A = int(g.integers(agents_range[0], agents_range[1] + 1)) if isinstance(agents_range, tuple) else int(agents_range)
    g.random(2 + A + 2 * T)
    st = g.bit_generator.state
    has = int(st["has_uint32"])
    words = [int(st["uinteger"])] if has else []
    for r in g.bit_generator.random_raw(T):
        words += [int(r) & 0xFFFFFFFF, int(r) >> 32]
    return A, T, has, words


def no_rejection_form(words, T, m):
    """What a generator that never rejects would give: word i makes requirement i."""
    return np.array([1 + ((w * m) >> 32) for w in words[:T]], np.int32)


# ---------------------------------------------------------------------------------------------------- np_stream.hpp on the host
SHIM = """
using namespace dcm::nps;
extern "C" {
// state and increment after seeding, as (hi, lo) pairs
void s_seed(uint64_t seed, uint64_t* out) {
    const Pcg p = pcg_seed(seed);
    out[0] = (uint64_t)(p.state >> 64); out[1] = (uint64_t)p.state; out[2] = (uint64_t)(p.inc >> 64); out[3] = (uint64_t)p.inc;
}
// a script of calls on one generator: kind[i] 0 = random(), 1 = integers(0, rng[i] + 1); returns the number of rejected words
uint32_t s_script(uint64_t seed, int n, const int32_t* kind, const uint32_t* rng, double* dout, uint32_t* iout) {
    Pcg p = pcg_seed(seed);
    uint32_t rejected = 0;
    for (int i = 0; i < n; i++) {
        if (kind[i] == 0) dout[i] = next_double(p);
        else iout[i] = bounded(p, rng[i], &rejected);
    }
    return rejected;
}
// k steps one by one against one jump: 1 when the states agree
int s_jump(uint64_t seed, uint64_t k) {
    Pcg p = pcg_seed(seed);
    const u128 jumped = jump(p.state, p.inc, jump_coeffs(k));
    for (uint64_t i = 0; i < k; i++) next64(p);
    return p.state == jumped ? 1 : 0;
}
// a lane's view: draw j of the stream taken by jump-ahead equals the j-th next64
int s_lane_draw(uint64_t seed, uint64_t j, uint64_t* by_jump, uint64_t* by_step) {
    Pcg p = pcg_seed(seed);
    *by_jump = output(jump(p.state, p.inc, jump_coeffs(j + 1)));
    uint64_t r = 0;
    for (uint64_t i = 0; i <= j; i++) r = next64(p);
    *by_step = r;
    return *by_jump == *by_step;
}
// generate_env (env/task_env.py:57-71) in stream order; returns T, *A_out = A
int s_generate(uint64_t seed, int a_lo, int a_hi, int t_lo, int t_hi, int m, double* depot, double* xy, int32_t* req, int* A_out) {
    Pcg p = pcg_seed(seed);
    const int T = t_lo + (int)bounded(p, (uint32_t)(t_hi - t_lo));
    const int A = a_lo + (int)bounded(p, (uint32_t)(a_hi - a_lo));
    depot[0] = next_double(p); depot[1] = next_double(p);
    for (int a = 0; a < A; a++) next_double(p);
    for (int i = 0; i < 2 * T; i++) xy[i] = next_double(p);
    for (int t = 0; t < T; t++) req[t] = 1 + (int32_t)bounded(p, (uint32_t)(m - 1));
    *A_out = A;
    return T;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """csrc/np_stream.hpp compiled with the host compiler into a small shim, asked through ctypes.  A test file that uses it imports
    it by name."""
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("np_stream")
    src, so = d / "np_stream_shim.cpp", d / "np_stream_shim.so"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "dcmrta_amd", "csrc", "np_stream.hpp") + SHIM)
    out = subprocess.run([cxx, "-std=c++17", "-O2", "-shared", "-fPIC", str(src), "-o", str(so)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lib = C.CDLL(str(so))
    lib.s_seed.argtypes = [C.c_uint64, C.c_void_p]
    lib.s_script.argtypes = [C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.s_script.restype = C.c_uint32
    lib.s_jump.argtypes = [C.c_uint64, C.c_uint64]
    lib.s_lane_draw.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.s_generate.argtypes = [C.c_uint64] + [C.c_int] * 5 + [C.c_void_p] * 4
    return lib


def shim_generate(lib, seed, a, t, m):
    """generate_env through the shim: (A, T, depot, task_xy padded to t[1], req padded to t[1])."""
    depot, xy, req, A = np.zeros(2), np.zeros((t[1], 2)), np.ones(t[1], np.int32), C.c_int()
    T = lib.s_generate(seed, a[0], a[1], t[0], t[1], m, depot.ctypes.data, xy.ctypes.data, req.ctypes.data, C.byref(A))
    return A.value, T, depot, xy, req
