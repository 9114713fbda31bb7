"""CPU: csrc/np_stream.hpp -- np.random.default_rng(seed) restated for the on-device instance generator -- against numpy itself and
against the reference's instances (tests/golden/instgen.npz, instances_ranges.json).  The header needs no HIP: it is compiled here
with the host compiler into a small shim and asked through ctypes.  Every comparison is exact."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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

SEEDS = list(range(1000)) + [2 ** 31 + 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 17, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 2 ** 31 + 5,
                             12345678901234567890, 2 ** 64 - 1]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
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


def _script(lib, seed, kind, rng):
    kind, rng = np.ascontiguousarray(kind, np.int32), np.ascontiguousarray(rng, np.uint32)
    dout, iout = np.zeros(len(kind)), np.zeros(len(kind), np.uint32)
    rej = lib.s_script(seed, len(kind), kind.ctypes.data, rng.ctypes.data, dout.ctypes.data, iout.ctypes.data)
    return dout, iout, rej


def test_seeding_state(shim):
    for s in SEEDS:
        st = np.random.PCG64(s).state["state"]
        out = (C.c_uint64 * 4)()
        shim.s_seed(s, out)
        assert (out[0] << 64 | out[1], out[2] << 64 | out[3]) == (st["state"], st["inc"]), s


def test_doubles(shim):
    for s in SEEDS:
        d, _, _ = _script(shim, s, [0] * 40, [0] * 40)
        assert np.array_equal(d, np.random.default_rng(s).random(40)), s


@pytest.mark.parametrize("bound", [5, 31, 3 * 2 ** 30, 2 ** 32 - 1])
def test_bounded_integers(shim, bound):
    rejected = 0
    for s in SEEDS:
        _, i, rej = _script(shim, s, [1] * 50, [bound - 1] * 50)
        assert np.array_equal(i, np.random.default_rng(s).integers(0, bound, 50).astype(np.uint32)), s
        rejected += rej
    if bound == 3 * 2 ** 30:
        # a quarter of all words is rejected at this bound: the redraw loop has run, and the results above depend on it
        assert rejected > 50 * len(SEEDS) // 8


def test_half_word_buffer_across_interleaved_calls(shim):
    """integers() takes half of a 64-bit draw and keeps the other half through any number of random() calls; integers(lo, lo + 1) draws
    nothing.  The call pattern of generate_env with one or two ranges is among these."""
    patterns = [[(1, 30), (0, 0), (0, 0), (1, 4), (1, 4), (1, 4)],                 # one size drawn: the first requirement takes the half
                [(1, 30), (1, 10), (0, 0), (1, 4), (1, 4)],
                [(1, 30), (1, 0), (0, 0), (1, 4), (0, 0), (1, 4), (1, 4), (0, 0), (1, 1000), (1, 0), (1, 7)],
                [(0, 0), (1, 15), (0, 0), (0, 0), (1, 15), (1, 3 * 2 ** 30 - 1), (0, 0), (1, 3 * 2 ** 30 - 1), (1, 2)]]
    for s in SEEDS:
        for pat in patterns:
            g = np.random.default_rng(s)
            want = [g.random() if k == 0 else int(g.integers(7, 7 + r + 1)) - 7 for k, r in pat]
            d, i, _ = _script(shim, s, [k for k, _ in pat], [r for _, r in pat])
            got = [d[n] if k == 0 else int(i[n]) for n, (k, _) in enumerate(pat)]
            assert got == want, (s, pat)


def test_jump_ahead_equals_stepping(shim):
    for s in SEEDS:
        for k in (0, 1, 2, 63, 64, 65, 122, 452, 1000, 2047, 4097):
            assert shim.s_jump(s, k) == 1, (s, k)
    a, b = C.c_uint64(), C.c_uint64()
    for s in SEEDS:
        raw = np.random.PCG64(s).random_raw(200)
        for j in (0, 1, 63, 64, 127, 199):
            assert shim.s_lane_draw(s, j, C.byref(a), C.byref(b)) == 1 and a.value == int(raw[j]), (s, j)


def _generate(lib, seed, a, t, m):
    depot, xy, req, A = np.zeros(2), np.zeros((t[1], 2)), np.ones(t[1], np.int32), C.c_int()
    T = lib.s_generate(seed, a[0], a[1], t[0], t[1], m, depot.ctypes.data, xy.ctypes.data, req.ctypes.data, C.byref(A))
    return A.value, T, depot, xy, req


def test_reference_instances(shim, golden_dir):
    """Every case of instgen.npz: TaskEnv(agents_range, tasks_range, max_coalition_size=m, seed=s) of the reference."""
    z = np.load(os.path.join(golden_dir, "instgen.npz"))
    n = 0
    for name in z["cases"]:
        a_lo, a_hi, _, t_lo, t_hi, _, m = (int(x) for x in z[f"{name}/params"])
        for i, s in enumerate(z[f"{name}/seeds"]):
            A, T, depot, xy, req = _generate(shim, int(s), (a_lo, a_hi), (t_lo, t_hi), m)
            assert (A, T) == (int(z[f"{name}/n_agents"][i]), int(z[f"{name}/n_tasks"][i])), (name, s)
            assert np.array_equal(depot, z[f"{name}/depot"][i]) and np.array_equal(xy, z[f"{name}/task_xy"][i]), (name, s)
            assert np.array_equal(req, z[f"{name}/req"][i]), (name, s)
            n += 1
    assert n > 200


def test_reference_instances_with_ranges(shim, golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "instances_ranges.json")))
    for sd, r in ref.items():
        A, T, depot, xy, req = _generate(shim, int(sd), (10, 20), (20, 50), 5)
        assert (A, T) == (r["A"], r["T"]) and depot.tolist() == r["depot"] and req[:T].tolist() == r["req"]
        assert xy[0].tolist() == r["task_xy0"] and xy[T - 1].tolist() == r["task_xy_last"]
