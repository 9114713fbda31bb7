"""CPU: tests/golden/rejecting_seeds.json (made by tests/golden/make_rejecting_seeds.py) holds seeds whose instance has a REJECTED
requirement word, i.e. seeds at which the on-device generator (csrc/instgen.hpp, wave_bounded) leaves its jump-ahead path for the
sequential routine.  The GPU tests that run that fall-back (tests/test_gpu_rejecting_seeds.py) rest on the fixture; this test proves
with numpy alone that every seed rejects where the fixture says, so that a fixture seed that does not reject is a failure here and
never a GPU case that quietly tests nothing.  Every comparison is exact."""
import numpy as np

from fixtures_ref import load_rejecting_seeds, no_rejection_form, numpy_words, shim, shim_generate  # noqa: F401  (shim: a fixture)

# classes the GPU cases need, with the fewest seeds each; the three 10-minute classes of the search are optional
NEEDED = {"m13_20A50T": 3, "m13_tasks_ranged_first_block": 2, "m13_tasks_ranged_later_block": 3, "m5_20A50T": 3,
          "m5_50A200T_later_block": 3, "m5_70A130T": 3, "m5_both_ranged": 3, "m5_100A500T_third_block_on": 3}
WINDOW = {"m13_tasks_ranged_first_block": (1, 127), "m13_tasks_ranged_later_block": (128, 299), "m5_50A200T_later_block": (128, 199),
          "m5_100A500T_third_block_on": (256, 499), "m13_tasks_ranged_buffered_half": (0, 0), "m13_tasks_ranged_word_127": (127, 127)}


def lemire_rejected(words, n, bound):
    """Indices of the rejected words among those that n values of integers(0, bound) consume, in Python integers."""
    threshold = ((1 << 32) - bound) % bound
    out, taken, i = [], 0, 0
    while taken < n:
        if ((words[i] * bound) & 0xFFFFFFFF) < threshold:
            out.append(i)
        else:
            taken += 1
        i += 1
    return out


def test_fixture_has_the_classes(golden_dir):
    fx = load_rejecting_seeds(golden_dir)
    for name, n in NEEDED.items():
        assert len(fx.get(name, [])) >= n, name
    seeds = [e["seed"] for entries in fx.values() for e in entries]
    assert all(0 <= s < 2 ** 64 for s in seeds)
    for name, (lo, hi) in WINDOW.items():
        for e in fx.get(name, []):
            assert lo <= e["first_rejected_word"] <= hi, (name, e["seed"])
    for name in fx:
        if name.startswith("m13_tasks_ranged"):
            for e in fx[name]:
                assert e["has"] == 1 and e["T"] > 128, e["seed"]   # the buffered half is carried across a block boundary
        else:
            assert all(e["has"] == 0 for e in fx[name]), name      # no size drawn, or both


def test_every_fixture_seed_rejects_where_recorded(golden_dir, shim):  # noqa: F811
    from dcmrta_amd.instances import generate_instance, generate_instance_ranges
    n = 0
    for name, entries in load_rejecting_seeds(golden_dir).items():
        for e in entries:
            ar, tr, m, s = e["agents_range"], e["tasks_range"], e["max_coalition_size"], e["seed"]
            A, T, has, words = numpy_words(s, ar, tr, m)
            rejected = lemire_rejected(words, T, m)
            assert (A, T, has) == (e["A"], e["T"], e["has"]), (name, s)
            assert rejected and rejected[0] == e["first_rejected_word"] and len(rejected) == e["rejections"], (name, s, rejected)
            # the host generator = numpy's own integers(): equal to the no-rejection form up to that word, different at it
            if isinstance(ar, tuple) or isinstance(tr, tuple):
                gA, inst = generate_instance_ranges(ar, tr, s, max_coalition_size=m)
                assert gA == A
            else:
                inst = generate_instance(A, T, s, max_coalition_size=m)
            req, w = inst["req"], e["first_rejected_word"]
            assert req.shape == (T,)
            closed = no_rejection_form(words, T, m)
            assert np.array_equal(req[:w], closed[:w]) and req[w] != closed[w], (name, s)
            # ... and so is the chain of nps::bounded calls, compiled for the host
            a2, t2 = (ar if isinstance(ar, tuple) else (ar, ar)), (tr if isinstance(tr, tuple) else (tr, tr))
            sA, sT, depot, xy, sreq = shim_generate(shim, s, a2, t2, m)
            assert (sA, sT) == (A, T) and np.array_equal(sreq[:T], req), (name, s)
            assert np.array_equal(depot, inst["depot"]) and np.array_equal(xy[:T], inst["task_xy"]), (name, s)
            n += 1
    assert n >= sum(NEEDED.values())
