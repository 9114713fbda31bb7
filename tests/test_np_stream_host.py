"""CPU: csrc/np_stream.hpp -- np.random.default_rng(seed) restated for the on-device instance generator -- against numpy itself and
against the reference's instances (tests/golden/instgen.npz, instances_ranges.json).  The header needs no HIP: it is compiled here
with the host compiler into a small shim (fixtures_ref.shim) and asked through ctypes.  Every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from fixtures_ref import shim, shim_generate  # noqa: F401  (shim: a fixture)

SEEDS = list(range(1000)) + [2 ** 31 + 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 17, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 2 ** 31 + 5,
                             12345678901234567890, 2 ** 64 - 1]


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


def test_reference_instances(shim, golden_dir):
    """Every case of instgen.npz: TaskEnv(agents_range, tasks_range, max_coalition_size=m, seed=s) of the reference."""
    z = np.load(os.path.join(golden_dir, "instgen.npz"))
    n = 0
    for name in z["cases"]:
        a_lo, a_hi, _, t_lo, t_hi, _, m = (int(x) for x in z[f"{name}/params"])
        for i, s in enumerate(z[f"{name}/seeds"]):
            A, T, depot, xy, req = shim_generate(shim, int(s), (a_lo, a_hi), (t_lo, t_hi), m)
            assert (A, T) == (int(z[f"{name}/n_agents"][i]), int(z[f"{name}/n_tasks"][i])), (name, s)
            assert np.array_equal(depot, z[f"{name}/depot"][i]) and np.array_equal(xy, z[f"{name}/task_xy"][i]), (name, s)
            assert np.array_equal(req, z[f"{name}/req"][i]), (name, s)
            n += 1
    assert n > 200


def test_reference_instances_with_ranges(shim, golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "instances_ranges.json")))
    for sd, r in ref.items():
        A, T, depot, xy, req = shim_generate(shim, int(sd), (10, 20), (20, 50), 5)
        assert (A, T) == (r["A"], r["T"]) and depot.tolist() == r["depot"] and req[:T].tolist() == r["req"]
        assert xy[0].tolist() == r["task_xy0"] and xy[T - 1].tolist() == r["task_xy_last"]
