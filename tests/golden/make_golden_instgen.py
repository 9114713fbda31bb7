#!/usr/bin/env python3
"""Problem instances of the reference generator, for the on-device generator (run in the build container only).

    python tests/golden/make_golden_instgen.py  ->  tests/golden/instgen.npz

Each case is TaskEnv(agents_range, tasks_range, 1, max_coalition_size=m, seed=s) of the reference (env/task_env.py:9-24,57-71) for a
list of seeds.  A range is stored as (lo, hi, is_tuple): an int range draws nothing, a tuple range draws the env's own size from
the seeded stream first (:58-65).  Per case `<name>/seeds` u64[N], `/n_agents`, `/n_tasks` i32[N], `/depot` f64[N,2], `/task_xy`
f64[N,Tmax,2], `/req` i32[N,Tmax], `/dur` f64[N,Tmax] -- rows beyond an env's own sizes padded with xy 0, req 1, dur 0 -- and
`/params` i64[7] = a_lo, a_hi, a_is_tuple, t_lo, t_hi, t_is_tuple, m.  `cases` lists the names.  Only numbers are stored.
"""
import os
import sys

import numpy as np

REF = os.environ.get("DCMRTA_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True

from env.task_env import TaskEnv  # noqa: E402  (reference, read-only)

OUT = os.path.dirname(os.path.abspath(__file__))
BIG = [2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 17, 2 ** 63, 2 ** 63 + 2 ** 31 + 5, 12345678901234567890, 2 ** 64 - 1]
SEEDS = list(range(32)) + BIG
FEW = list(range(8)) + [2 ** 32 + 12345, 2 ** 63 + 2 ** 31 + 5]

# name, agents_range, tasks_range, max_coalition_size, seeds
CASES = [
    ("fixed_20A50T", 20, 50, 5, SEEDS),
    ("both_ranges", (10, 20), (20, 50), 5, SEEDS),
    ("tasks_ranged", 15, (20, 50), 5, SEEDS),
    ("agents_ranged", (10, 20), 40, 5, SEEDS),
    ("zero_width_tuples", (20, 20), (50, 50), 5, FEW),
    ("fixed_m1", 20, 50, 1, FEW), ("fixed_m3", 20, 50, 3, FEW), ("fixed_m16", 20, 50, 16, FEW),
    ("both_m1", (10, 20), (20, 50), 1, FEW), ("both_m3", (10, 20), (20, 50), 3, FEW), ("both_m16", (10, 20), (20, 50), 16, FEW),
    ("tasks_m1", 15, (20, 50), 1, FEW), ("tasks_m3", 15, (20, 50), 3, FEW), ("tasks_m16", 15, (20, 50), 16, FEW),
    ("agents_m16", (10, 20), 40, 16, FEW),
    ("fixed_50A200T", 50, 200, 5, [0]),
    ("fixed_100A500T", 100, 500, 5, [0]),
]


def bounds(r):
    return (int(r[0]), int(r[1]), 1) if isinstance(r, tuple) else (int(r), int(r), 0)


def main():
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, ar, tr, m, seeds in CASES:
        a, t = bounds(ar), bounds(tr)
        N, Tm = len(seeds), t[1]
        depot, xy = np.zeros((N, 2)), np.zeros((N, Tm, 2))
        req, dur = np.ones((N, Tm), np.int32), np.zeros((N, Tm))
        na, nt = np.zeros(N, np.int32), np.zeros(N, np.int32)
        for i, s in enumerate(seeds):
            env = TaskEnv(ar, tr, 1, m, seed=s)
            T, A = env.tasks_num, env.agents_num
            na[i], nt[i] = A, T
            depot[i] = np.asarray(env.depot["location"], dtype=np.float64)
            for k in range(T):
                xy[i, k] = np.asarray(env.task_dic[k]["location"], dtype=np.float64)
                req[i, k] = int(env.task_dic[k]["requirements"][0])
                dur[i, k] = float(env.task_dic[k]["time"])
        out.update({f"{name}/seeds": np.array(seeds, dtype=np.uint64), f"{name}/n_agents": na, f"{name}/n_tasks": nt,
                    f"{name}/depot": depot, f"{name}/task_xy": xy, f"{name}/req": req, f"{name}/dur": dur,
                    f"{name}/params": np.array([*a, *t, m], dtype=np.int64)})
    np.savez_compressed(os.path.join(OUT, "instgen.npz"), **out)
    print("instgen.npz: %d cases, %d instances" % (len(CASES), sum(len(c[4]) for c in CASES)))


if __name__ == "__main__":
    main()
