"""The kernel families at non-default time limits and on degenerate instances (test infrastructure): the form table that
test_gpu_param_edges.py and test_param_edges_host.py share -- every shape under every (max_waiting_time, max_time) set, the degenerate
instances at the reference's 10 / 100, and two budgeted rows at the smallest positive waiting time -- and what the oracle alone says
about each case: how its episodes end, how often its agents are abandoned, where `nearest` meets equal distances."""
import functools

import numpy as np

import lookahead_ref as LA
import oracle_ref as O
from forms import Forms

# id: (A, T, B, BatchedTaskEnv keywords, ragged ranges); the kernel a random launch with all or no observation buffers takes (plan.hpp)
SHAPES = {
    "small": (6, 12, 8, {}, None),                                      # Fast, Sim<20,50,RS>
    "few-agents": (3, 12, 8, {}, None),                                 # the same; requirements 4 and 5 can never be met
    "exact": (20, 50, 6, {}, None),                                     # Fast, Sim<20,50>: compile-time sizes
    "ragged": (20, 50, 6, {}, ((10, 20), (20, 50))),                    # Fast, runtime sizes
    "lay64": (30, 60, 4, {}, None),                                     # Fast, Lay{64,64}
    "no-depot-lane": (10, 64, 4, {}, None),                             # General, Sim<64,64,RS>: T = 64 leaves no lane for the depot
    "mid": (66, 70, 4, {}, None),                                       # FastG, two agent chunks
    "mc": (50, 200, 2, {}, None),                                       # FastMc
    "chunks": (6, 130, 4, {}, None),                                    # FastG, three task chunks
    "wide": (10, 20, 4, dict(member_cap=16), None),                     # General, RuntimeWide
    "many-agents": (70, 6, 4, {}, None),                                # FastG, A far above T
}
# (max_waiting_time, max_time): the limit cuts episodes with work left; many abandonments (the 16-entry log overflows into the dense
# table); in between; nobody is ever abandoned for waiting (the float wake-up bound sits where a float's spacing is 1/16)
PARAMS = {"w10-t30": (10.0, 30.0), "w3-t250": (3.0, 250.0), "w25-t100": (25.0, 100.0), "w1e6-t100": (1e6, 100.0)}
DEGENERATE_SHAPES = ("small", "few-agents", "no-depot-lane", "mc", "wide")
TINY_SHAPES = ("small", "mc")                                           # max_waiting_time 1e-9 under a scalar budget of 200 decisions
TINY_MWT, TINY_BUDGET = 1e-9, 200
UNIFORM_BASE, RAGGED_BASE, CHOICE_BASE = 9000, 9100, 53


def form_id(shape, params):
    return f"{shape}-{params}"


def table():
    forms = {}
    for s, (A, T, B, kw, ranges) in SHAPES.items():
        for p, (mwt, mt) in PARAMS.items():
            forms[form_id(s, p)] = (A, T, B, dict(kw, max_waiting_time=mwt, max_time=mt), ranges, -1)
    for s in DEGENERATE_SHAPES:
        A, T, B, kw, ranges = SHAPES[s]
        forms[form_id(s, "degenerate")] = (A, T, B, dict(kw, max_waiting_time=10.0, max_time=100.0), ranges, -1)
    for s in TINY_SHAPES:
        A, T, B, kw, ranges = SHAPES[s]
        forms[form_id(s, "tiny")] = (A, T, B, dict(kw, max_waiting_time=TINY_MWT, max_time=100.0), ranges, TINY_BUDGET)
    return forms


FORMS = table()
F = Forms(FORMS, {}, UNIFORM_BASE, RAGGED_BASE, CHOICE_BASE, degenerate=[form_id(s, "degenerate") for s in DEGENERATE_SHAPES])


def params_of(form):
    kw = FORMS[form][3]
    return kw["max_waiting_time"], kw["max_time"]


def sizes(form):
    """(a, t) per env"""
    A, T, B, _, ranges, _ = FORMS[form]
    inst, _ = F.instances(form)
    return [(A, T)] * B if ranges is None else [(int(inst["n_agents"][b]), int(inst["n_tasks"][b])) for b in range(B)]


def ending(o, max_time):
    """How the episode an OracleEnv holds ended: "finished" (every task finished, every agent back), "max-time" (the clock reached
    max_time with work left) or "stuck" (work left, the clock short of max_time and nobody left to decide: the oracle's guard)."""
    f = o.final()
    if f["finished"].all() and f["returned"].all():
        return "finished"
    if o.now >= max_time:
        return "max-time"
    assert f["truncated"], "an episode that is neither finished nor at max_time ends under the guard"
    return "stuck"


def abandonments(o):
    """int64[A]: how often each agent was abandoned in the episode an OracleEnv holds"""
    n = np.zeros(o.A, np.int64)
    for t in range(o.T):
        n += np.bincount(o.abandoned(t), minlength=o.A)
    return n


@functools.lru_cache(maxsize=None)
def facts(form, policy, episodes=3):
    """Per env and episode of a form under a policy (forms.Forms.episodes: unlimited launches of one episode each)
    dict(ending, abandoned: int64[a])."""
    mt = params_of(form)[1]
    return [[dict(ending=ending(e.o, mt), abandoned=abandonments(e.o)) for e in eps] for eps in F.episodes(form, policy, episodes)]


@functools.lru_cache(maxsize=None)
def nearest_ties(form):
    """Per env of a form: the decisions of its first `nearest` episode (the oracle's recorded rollout) at which two unmasked tasks lie at
    one rounded distance from the deciding agent and no unmasked task lies nearer -- a tie that the lowest-index rule decides."""
    inst, seeds = F.instances(form)
    mwt, mt = params_of(form)
    out = []
    for b, (a, t) in enumerate(sizes(form)):
        one = O.one(inst, b, t)
        r = O.episodes(a, t, one, seeds[b], "nearest", 1, mwt, record=True, max_time=mt)[0]
        depot = (float(one["depot"][0]), float(one["depot"][1]))
        pos, ties = [depot] * a, []
        for d in range(r["n_steps"]):
            leader, act = int(r["leader"][d]), int(r["action"][d])
            free = np.flatnonzero(r["mask"][d][1:] == 0)
            dist = [LA.distance(pos[leader][0], pos[leader][1], one["task_xy"][k, 0], one["task_xy"][k, 1]) for k in free]
            if len(dist) >= 2 and dist.count(min(dist)) >= 2:
                ties.append(d)
                assert act == int(free[dist.index(min(dist))]) + 1, "the oracle's `nearest` takes the lowest index of a tie"
            to = depot if act == 0 else (float(one["task_xy"][act - 1, 0]), float(one["task_xy"][act - 1, 1]))
            for m in [leader] + [int(x) for x in r["followers"][d][:int(r["nfol"][d])]]:
                pos[m] = to
        out.append(ties)
    return out


# ---------------------------------------------------------------------------------- what a case must exercise (from the oracle alone)
POLICIES = ("random", "first", "nearest")
CUT_EVERYWHERE = ("small", "exact", "lay64", "no-depot-lane", "mc", "chunks", "wide")      # at max_time 30 no env finishes, any policy
AB_CAP = 16                                     # entries of an agent's abandonment log (csrc/common.hpp); further ones: the count table
OVERFLOWING = tuple(s for s in SHAPES if s not in ("many-agents", "mid"))                   # some agent is abandoned more than AB_CAP times


def split(form):
    shape = next(s for s in sorted(SHAPES, key=len, reverse=True) if form.startswith(s + "-"))
    return shape, form[len(shape) + 1:]


def check_case(form, policy):
    """The conditions under which a form's launches under a policy reach the path they are there for; counted on the CPU, from the
    oracle's episodes alone (DESIGN.md section 4 has the counts)."""
    shape, params = split(form)
    if params == "tiny":
        sims, steps = F.sims(form, policy, 3)
        assert (steps == TINY_BUDGET).all() and not any(s.done for s in sims), (form, policy, "the budget must stop every env in mid-episode")
        return
    fa = facts(form, policy)
    ends = [e["ending"] for env in fa for e in env]
    most = max(int(e["abandoned"].max()) for env in fa for e in env)
    mwt, mt = params_of(form)
    if params == "w10-t30":
        if shape in CUT_EVERYWHERE:
            assert set(ends) == {"max-time"}, (form, policy, ends)
        if shape == "mid":                      # 66 agents for 70 tasks: some envs finish inside 30 under the greedy policies
            assert "max-time" in ends and (policy == "random" or "finished" in ends), (form, policy, ends)
    if params == "w3-t250" and policy == "random":
        if shape in OVERFLOWING:
            assert most > AB_CAP, (form, most)
        if shape == "mc":
            assert max(int(e["abandoned"].sum()) for env in fa for e in env) > 1000, form
    if params == "w1e6-t100" and policy == "random":
        # nobody waits 1e6: the only abandonments are those of a coalition that overfills (a handful), and an env whose agents all
        # wait has its clock jump to the first wake-up, arrival + 1e6 -- the episode ends there, behind max_time, with work left
        assert max(int(e["abandoned"].sum()) for env in fa for e in env) <= 8, form
        jumped = [e.o.now >= mwt for eps in F.episodes(form, policy, 3) for e in eps]
        assert any(jumped) or shape in ("mid", "many-agents"), (form, "no env's clock jumps to a wake-up at arrival + 1e6")
    if params == "degenerate" and policy == "nearest":
        assert all(len(t) >= 1 for t in nearest_ties(form)), (form, [len(t) for t in nearest_ties(form)])


def expected_flags(f):
    """the env's header flags after an episode with the oracle's terminal results f: DONE, FINISHED, TRUNCATED (the guard)"""
    return 1 | (2 if f["finished"].all() and f["returned"].all() else 0) | (4 if f["truncated"] else 0)


# ---------------------------------------------------------------------------------- shared references, each computed once
@functools.lru_cache(maxsize=None)
def first_lengths(form, policy):
    """decisions of every env's first episode"""
    mwt, mt = params_of(form)
    inst, seeds = F.instances(form)
    return [O.episodes(a, t, O.one(inst, b, t), seeds[b], policy, 1, mwt, max_time=mt)[0]["n_steps"] for b, (a, t) in enumerate(sizes(form))]


@functools.lru_cache(maxsize=None)
def handover_walks(form):
    """removal_ref.walk_episode of every env's first random episode: the snapshots in front of every decision (sparse abandonment tables)"""
    import oracle
    import removal_ref as RR
    mwt, mt = params_of(form)
    inst, seeds = F.instances(form)
    out = []
    for b, (a, t) in enumerate(sizes(form)):
        o = oracle.OracleEnv(a, t, max_waiting_time=mwt, max_time=mt).load(**O.one(inst, b, t))
        out.append(RR.sparse_abandoned(RR.walk_episode(o, inst["req"][b], int(seeds[b]), mt)[0]))
    return out


Q25 = 1 << 30                                   # choice.explore_q32(0.25)


@functools.lru_cache(maxsize=None)
def explore_cases(form, episodes=3):
    """explore_ref.explore_episodes of every env: `nearest` at epsilon 0.25"""
    import explore_ref as EX
    mwt, mt = params_of(form)
    inst, seeds = F.instances(form)
    return [EX.explore_episodes(a, t, O.one(inst, b, t), int(seeds[b]), "nearest", Q25, episodes, mwt, mt) for b, (a, t) in enumerate(sizes(form))]


def kept(eps):
    """the index of the episode the best log keeps of an env's episodes: the largest (finished tasks, reward), the earliest of a tie"""
    best = 0
    for k in range(1, len(eps)):
        if LA.pair(eps[k]["result"]) > LA.pair(eps[best]["result"]):
            best = k
    return best


@functools.lru_cache(maxsize=None)
def double_drops(form, policy, episodes=3):
    """Per env of a form, over the decisions of one launch of `episodes` episodes under the form's budget: the (agent, tasks) of every
    task_update pass in which ONE agent was moved to the abandoned list of two or more tasks.  An agent gets there by deciding while a
    task still lists it -- it wakes at arrival + max_waiting_time, and the rounded difference now - arrival is still below
    max_waiting_time -- and joining another task.  The abandonment log keeps an agent's entries in event order; the order of the
    entries of one pass is not defined (every reader sorts the row), and the kernel families differ in it."""
    import lookahead_policy_ref as LP
    mwt, mt = params_of(form)
    inst, seeds = F.instances(form)
    budget = FORMS[form][5]
    out = []
    for b, (a, t) in enumerate(sizes(form)):
        found, d0, left = [], 0, (budget if budget >= 0 else None)
        for _ in range(episodes):
            if left == 0:
                break
            nab = np.zeros(t, np.int64)

            def after(o):
                now = o.final()["n_abandoned"]
                who = {}
                for k in np.flatnonzero(now != nab):
                    for agent in o.abandoned(int(k))[nab[k]:]:
                        who.setdefault(int(agent), []).append(int(k))
                found.extend((agent, tasks) for agent, tasks in who.items() if len(tasks) > 1)
                nab[:] = now

            w = LA.walk(a, t, O.one(inst, b, t), LP.shifted_seed(seeds[b], d0),
                        lambda c: LA.base_pick(policy, c.seed_of)(c.mask, c.pos, c.task_xy, c.d), mwt, stop=left, max_time=mt, after_task_update=after)
            d0 += w["n_steps"]
            left = None if left is None else left - w["n_steps"]
        out.append(found)
    return out


LOOKAHEAD_WINDOW_K = 4                          # at w3-t250 a whole lookahead episode costs the CPU walker a minute: a window instead


@functools.lru_cache(maxsize=None)
def lookahead_cases(form, width):
    """Per env of a form under rollout("nearest", lookahead=True[, width]).  Whole episodes (dict(whole=True, w: LP.lookahead_walk's or
    LW.width_walk's)) except at w3-t250, where `nearest` plays the first half of its own episode, the lookahead rule the next
    LOOKAHEAD_WINDOW_K decisions and `nearest` the rest (dict(whole=False, d0, window: the window's walk, tail: LP.window_tail's))."""
    import lookahead_policy_ref as LP
    import lookahead_width_ref as LW
    mwt, mt = params_of(form)
    inst, seeds = F.instances(form)
    whole = split(form)[1] != "w3-t250"
    out = []
    for b, (a, t) in enumerate(sizes(form)):
        one, seed = O.one(inst, b, t), int(seeds[b])
        if whole:
            w = LP.lookahead_walk(a, t, one, seed, "nearest", mwt, mt) if width is None else LW.width_walk(a, t, one, seed, "nearest", width, mwt, mt)
            out.append(dict(whole=True, w=w))
        else:
            d0 = first_lengths(form, "nearest")[b] // 2
            win = LP.lookahead_window(a, t, one, seed, "nearest", mwt, d0, LOOKAHEAD_WINDOW_K, mt) if width is None else \
                LW.width_window(a, t, one, seed, "nearest", mwt, width, d0, LOOKAHEAD_WINDOW_K, mt)
            out.append(dict(whole=False, d0=d0, window=win, tail=LP.window_tail(a, t, one, seed, "nearest", mwt, win["chosen"], mt)))
    return out


@functools.lru_cache(maxsize=None)
def fork_points(form, share=0.75):
    """per env: the decisions of the first random episode in front of the fork, and the most abandonments of one agent by then"""
    mwt, mt = params_of(form)
    inst, seeds = F.instances(form)
    at = [max(1, int(share * n)) for n in first_lengths(form, "random")]
    most = [int(abandonments(O.play(a, t, O.one(inst, b, t), seeds[b], 0, "random", at[b], mwt, mt)[0]).max()) for b, (a, t) in enumerate(sizes(form))]
    return at, most
