"""-m gpu: dcm_fork_envs (BatchedTaskEnv.fork_from) -- env b of a destination handle becomes env src_index[b] of a source handle.

Six source envs are brought to different places of their episodes -- fresh after reset, stopped by a budget under random and under
nearest, advanced by dcm_step, DONE -- and copied into thirteen destination envs under a map with duplicates, a permutation and -1s.
  1. byte exactness: every copied row of the four sections of the dcm_clone_state blob is the source's row, every other row is what it
     was, a new seed changes the eight bytes of the header's seed and nothing else, ok_out is as specified;
  2. continuation: copy and source, continued by the same call of every rollout family the shape has and by dcm_step, give the same
     steps, records, summary rows and observation stores, to the end of the episode; a copy with a new seed plays the oracle's episode
     with the seed of the draws switched at that decision (lookahead_ref.walk);
  3. in place: a valid map, the seed-only change at s == b, and the refuse-and-skip path for maps that break the source rule or leave
     the range (those envs are never written and never read: nothing can race);
  4. every host-side refusal, with both handles byte-identical afterwards; the restart image a destination had; renewal afterwards."""
import numpy as np
import pytest

import helpers as H
import lookahead_ref as LA
import oracle_ref as O

B_SRC, B_DST = 6, 13
INST_SEED, CHOICE_SEED = 23, 7
ERR_INVALID, ERR_STATE = -1, -4
LOG_CAP = 64
# env b of dst <- env MAP[b] of src: 0..5 each at least once (a permutation of the sources sits in it), duplicates, two -1s
MAP = np.array([3, 0, 0, -1, 5, 1, 2, 4, 4, 1, -1, 2, 5], np.int32)
# where the sources are brought to.  k: decisions taken by the budget-stopped envs 1 (random), 2 (nearest), 5 (random, deeper)
PLACES = ("fresh", "random", "nearest", "step", "done", "random")
# legs: what continues copy and source -- P / Pn: a persistent launch with all / no observation buffers, G: with the mask alone (the
# general kernel at every shape), L: with the rollout log, X: epsilon-greedy, B: best-keeping, S: dcm_step in its plain call shape,
# Sg: with an injected leader (the general kernel).  The shapes' families are those of test_gpu_relay.py, without the renewing ones
CASES = {
    "one": dict(A=20, T=50, mwt=2.0, k=(7, 5, 15), legs="P Pn G L X B S Sg"),            # Lay{20,50}, register-resident
    "lay64": dict(A=30, T=60, mwt=2.0, k=(7, 5, 15), legs="P Pn G L X B S Sg"),          # Lay{64,64}
    "g2x3": dict(A=70, T=130, mwt=1.0, k=(9, 6, 30), legs="P Pn L X B S"),               # mid-size, multi-chunk
    "mc": dict(A=50, T=200, mwt=1.5, k=(9, 6, 30), legs="P Pn L X B S"),                 # 50A/200T
    "wide": dict(A=24, T=9, mwt=2.0, k=(2, 2, 4), legs="P L X B S", req=16, member_cap=16),   # DCM_PARAM_WIDE_MEMBERS
}
LEGS = {"P": dict(obs="all"), "Pn": dict(obs="none"), "G": dict(obs="mask"), "L": dict(obs="all", log=True), "X": dict(obs="all", explore=True),
        "B": dict(obs="all", log=True, best=True), "S": dict(step="plain"), "Sg": dict(step="leader")}

_inst = {}


def instances(name, which="src"):
    """(instances, choice seeds) of a case's source handle, or of its destination's own batch (other instances, other seeds)"""
    from dcmrta_amd.choice import env_seeds
    from dcmrta_amd.instances import generate_batch
    if (name, which) not in _inst:
        c = CASES[name]
        B, base = (B_SRC, INST_SEED) if which == "src" else (B_DST, INST_SEED + 100)
        inst = generate_batch(B, c["A"], c["T"], base_seed=base + c["A"])
        if c.get("req"):
            inst["req"] = np.random.default_rng(base).integers(1, c["req"] + 1, (B, c["T"])).astype(np.int32)
        _inst[name, which] = (inst, env_seeds(CHOICE_SEED + (which != "src"), 0, B))
    return _inst[name, which]


@pytest.mark.parametrize("name", list(CASES))
def test_the_sources_places_exist(oracle_lib, name):
    """CPU: the budgets of the preparation stop envs 1, 2 and 5 in mid-episode, with decisions to spare for the continuation legs"""
    c = CASES[name]
    inst, seeds = instances(name)
    for b, policy, k in ((1, "random", c["k"][0]), (2, "nearest", c["k"][1]), (5, "random", c["k"][2])):
        n = O.episodes(c["A"], c["T"], O.one(inst, b), seeds[b], policy, 1, c["mwt"])[0]["n_steps"]
        assert n >= k + 4, (name, b, n, k)
    assert sorted(set(MAP.tolist())) == [-1, 0, 1, 2, 3, 4, 5] and len(MAP) == B_DST and len(PLACES) == B_SRC
    assert any((MAP == s).sum() >= 2 for s in range(B_SRC))


# ---------------------------------------------------------------------------------------------------------------- blobs
def sections(env, blob=None):
    """The dcm_clone_state blob of a uniform batch as its four sections, one row per env: the records, the summary rows, the
    abandonment logs u16[A][16] and the overflow count tables u16[A][T] in their 16-byte padded pitch."""
    blob = (env.clone_state() if blob is None else blob).cpu().numpy()
    B, rec, pitch = env.B, env.record_bytes(), (2 * env.A * env.T + 15) // 16 * 16
    sizes = [B * rec, B * 64, B * env.A * 32, B * pitch]
    assert blob.size == sum(sizes)
    parts = np.split(blob, np.cumsum(sizes)[:-1])
    return {k: p.reshape(B, -1).copy() for k, p in zip(("record", "summary", "ablog", "abcnt"), parts)}


def blob_of(env, sec):
    import torch
    return torch.from_numpy(np.concatenate([sec[k].ravel() for k in ("record", "summary", "ablog", "abcnt")])).to(env.device)


def assert_rows(got, want, rows_got, rows_want, tag):
    for k in want:
        assert got[k][rows_got].tobytes() == want[k][rows_want].tobytes(), (tag, k)


def first_free(mask):
    """the lowest unmasked action of every env (0 where there is none)"""
    return np.argmax(np.asarray(mask) == 0, axis=1).astype(np.int32)


def make_env(gpu_device, name, B, **kw):
    from dcmrta_amd.batched_env import BatchedTaskEnv
    c = CASES[name]
    return BatchedTaskEnv(B, c["A"], c["T"], device=gpu_device, max_waiting_time=c["mwt"], member_cap=c.get("member_cap", 5), **kw)


def source(gpu_device, name):
    """(the source handle with its six envs at PLACES, its blob sections).  The places are put together row by row from snapshots of
    one handle, through dcm_restore_state: dcm_step and the persistent launches move every env that can move."""
    c = CASES[name]
    inst, seeds = instances(name)
    env = make_env(gpu_device, name, B_SRC).load_instances(**inst)
    env.reset(seeds, observe=False)
    fresh = sections(env)
    k1, k2, k5 = c["k"]
    big = 1 << 40
    s1 = env.rollout("random", write_obs=False, max_decisions=np.array([0, k1, 0, 0, big, k5], np.int64)).cpu().numpy()
    s2 = env.rollout("nearest", write_obs=False, max_decisions=np.array([0, 0, k2, 0, 0, 0], np.int64)).cpu().numpy()
    assert s1[[0, 1, 2, 3, 5]].tolist() == [0, k1, 0, 0, k5] and s1[4] > k5 and s2.tolist() == [0, 0, k2, 0, 0, 0]
    mid = sections(env)
    env.step(first_free(env.observe().mask.cpu().numpy()))
    stepped = sections(env)
    sec = {k: mid[k].copy() for k in mid}
    for k in sec:
        sec[k][0] = fresh[k][0]
        sec[k][3] = stepped[k][3]
    env.restore_state(blob_of(env, sec))
    st = env.status()
    assert st["decisions"].cpu().numpy()[[0, 1, 2, 3, 5]].tolist() == [0, k1, k2, 1, k5]
    assert (st["flags"].cpu().numpy() & 1).tolist() == [0, 0, 0, 0, 1, 0]
    assert sections(env)["record"].tobytes() == sec["record"].tobytes()
    return env, sec


def destination(gpu_device, name, **kw):
    """a destination handle on its own instances, reset and a few random decisions into its own episodes"""
    inst, seeds = instances(name, "dst")
    env = make_env(gpu_device, name, B_DST, **kw).load_instances(**inst)
    env.reset(seeds, observe=False)
    env.rollout("random", write_obs=False, max_decisions=2)
    return env


def fork_raw(dst, src, index, seeds=None, with_ok=True):
    """dcm_fork_envs itself: (return code, message, ok_out as numpy or None)"""
    import torch
    from dcmrta_amd.batched_env import _ptr
    idx = None if index is None else torch.as_tensor(np.asarray(index, np.int32)).to(dst.device)
    s = None if seeds is None else torch.from_numpy(np.ascontiguousarray(seeds, np.uint64).view(np.int64)).to(dst.device)
    ok = torch.full((dst.B,), 7, dtype=torch.uint8, device=dst.device) if with_ok else None
    with torch.cuda.device(dst.device):
        rc = dst._lib.dcm_fork_envs(dst._h, None if src is None else src._h, _ptr(idx), _ptr(s), _ptr(ok), dst._stream())
        torch.cuda.synchronize(dst.device)
    msg = dst._lib.dcm_last_error()
    return rc, (msg.decode() if msg else ""), (None if ok is None else ok.cpu().numpy())


def seed_bytes(seeds):
    return np.ascontiguousarray(seeds, np.uint64).view(np.uint8).reshape(-1, 8)


# ---------------------------------------------------------------------------------------------------------------- 1. byte exactness
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_copied_rows_are_the_sources_bytes(gpu_device, name):
    src, ssec = source(gpu_device, name)
    dst = destination(gpu_device, name)
    before = sections(dst)
    copied, alone = np.flatnonzero(MAP >= 0), np.flatnonzero(MAP < 0)
    rc, msg, ok = fork_raw(dst, src, MAP)
    assert rc == 0 and ok.tolist() == [1] * B_DST, (rc, msg, ok)
    after = sections(dst)
    assert_rows(after, ssec, copied, MAP[copied], "copied rows")
    assert_rows(after, before, alone, alone, "rows left alone")
    assert_rows(sections(src), ssec, slice(None), slice(None), "the source")
    # ... through fork_from, with new seeds: only the seed field of the copied envs differs
    new = np.arange(B_DST, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1 << 63)
    assert dst.fork_from(src, MAP, seeds=new, check=True) is dst
    seeded = sections(dst)
    want = {k: after[k].copy() for k in after}
    want["record"][copied, 8:16] = seed_bytes(new)[copied]
    assert_rows(seeded, want, slice(None), slice(None), "with seeds_in")
    assert not np.array_equal(seeded["record"][copied, 8:16], after["record"][copied, 8:16])
    # ok_out may be NULL, and an index outside [-1, B_src) between two handles refuses that env alone
    wild = MAP.copy()
    wild[[2, 7]] = [B_SRC, -2]
    rc, msg, ok = fork_raw(dst, src, wild)
    assert rc == 0 and ok.tolist() == [0 if b in (2, 7) else 1 for b in range(B_DST)], (rc, msg, ok)
    assert_rows(sections(dst), seeded, [2, 7], [2, 7], "refused rows")
    rc, msg, _ = fork_raw(dst, src, MAP, with_ok=False)
    assert rc == 0, msg
    assert_rows(sections(dst), after, slice(None), slice(None), "without ok_out")
    src.close(); dst.close()


# ---------------------------------------------------------------------------------------------------------------- 2. continuation
def run_leg(env, leg, budget):
    """one call of a leg on a handle: (steps int64[B] or None, what the call stored: the observation buffers it writes)"""
    import torch
    from dcmrta_amd import _lib
    from dcmrta_amd.batched_env import _ptr, check
    l = LEGS[leg]
    if "step" in l:
        obs = env.observe()
        act = first_free(obs.mask.cpu().numpy())
        if l["step"] == "plain":                            # the plain call shape: a contiguous int32 tensor on the device, nothing else
            o = env.step(torch.from_numpy(act).to(env.device))
        else:
            o = env.step(act, leader=np.full(env.B, -1, np.int32))
        return None, [x.cpu().numpy().copy() for x in (o.agents, o.tasks, o.mask, o.leader, o.active)]
    env.enable_rollout_log(LOG_CAP if l.get("log") else 0)
    if l.get("best"):
        env.enable_best_log()
    per = np.full(env.B, budget, np.int64)
    if l["obs"] == "mask":
        steps = torch.empty((env.B,), dtype=torch.int64, device=env.device)
        d = env._dev(per, torch.int64)
        with torch.cuda.device(env.device):
            check(env._lib.dcm_rollout_random(env._h, 1, -1, _ptr(d), None, None, _ptr(env._mask), _ptr(steps), env._stream()))
        stored = [env._mask.cpu().numpy().copy()]
    else:
        kw = dict(explore=0.5) if l.get("explore") else {}
        steps = env.rollout("nearest" if l.get("explore") or l.get("best") else "random", episodes=1, write_obs=l["obs"] == "all", max_decisions=per, **kw)
        o = env.obs()
        stored = [x.cpu().numpy().copy() for x in (o.agents, o.tasks, o.mask)] if l["obs"] == "all" else []
    if l.get("best"):
        env.enable_best_log(False)
    env.enable_rollout_log(0)
    return steps.cpu().numpy(), stored


def after_leg(env):
    st = env.status()
    return dict(sections(env), flags=st["flags"].cpu().numpy(), decisions=st["decisions"].cpu().numpy(), now=st["now"].cpu().numpy(),
                episodes=env.episodes().cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_copy_and_source_continue_alike(gpu_device, name):
    src, ssec = source(gpu_device, name)
    dst = destination(gpu_device, name)
    sblob = blob_of(src, ssec)
    copied = np.flatnonzero(MAP >= 0)
    for leg in CASES[name]["legs"].split():
        src.restore_state(sblob)
        dst.fork_from(src, MAP, check=True)
        # the leg itself: three decisions (a DONE env restarts and plays three of its next episode), or one dcm_step
        got = [run_leg(e, leg, 3) for e in (dst, src)]
        (dsteps, dstored), (ssteps, sstored) = got
        if dsteps is not None:
            assert np.array_equal(dsteps[copied], ssteps[MAP[copied]]), (leg, "steps")
        for x, y in zip(dstored, sstored):
            assert x[copied].tobytes() == y[MAP[copied]].tobytes(), (leg, "observation stores")
        d, s = after_leg(dst), after_leg(src)
        assert_rows(d, s, copied, MAP[copied], leg)
        # ... and on to the end of the episode each env is in
        dsteps, ssteps = (e.rollout("nearest", episodes=1, write_obs=False).cpu().numpy() for e in (dst, src))
        assert np.array_equal(dsteps[copied], ssteps[MAP[copied]]), (leg, "steps to the end")
        d, s = after_leg(dst), after_leg(src)
        assert_rows(d, s, copied, MAP[copied], leg + " to the end")
        assert (d["flags"][copied] & 1).all() and not np.isnan(d["summary"].view(np.float64)[copied]).any(), leg
    src.close(); dst.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_a_copy_with_a_new_seed_plays_the_walk_with_the_seed_switched(gpu_device, oracle_lib, name):
    """sources 0 (fresh), 1 (k decisions of random) and 2 (k decisions of nearest), copied with new seeds and played on to the end under
    the policy that brought them there: the oracle's episode with the seed of the draws switched at that decision; a copy that keeps
    the seed plays the source's own episode"""
    c = CASES[name]
    A, T, mwt = c["A"], c["T"], c["mwt"]
    inst, seeds = instances(name)
    src, _ = source(gpu_device, name)
    dst = destination(gpu_device, name)
    new = np.array([0xDEADBEEF12345678 + 977 * b for b in range(B_DST)], np.uint64)
    for policy, rows in (("nearest", {0: (0, 0), 1: (2, c["k"][1]), 2: (0, 0)}), ("random", {0: (1, c["k"][0]), 1: (5, c["k"][2]), 2: (1, c["k"][0])})):
        idx = np.full(B_DST, -1, np.int32)
        for b, (s, _) in rows.items():
            idx[b] = s
        dst.fork_from(src, idx, seeds=new, check=True)
        keep = np.where(np.arange(B_DST) == 2, idx, -1).astype(np.int32)       # env 2 once more, without a new seed
        dst.fork_from(src, keep, check=True)
        dst.rollout(policy, episodes=1, write_obs=False, max_decisions=np.where(idx >= 0, -1, 0).astype(np.int64))
        sm = dst.summary().cpu().numpy()
        for b, (s, k) in rows.items():
            switch = None if b == 2 else (k, int(new[b]))
            w = LA.policy_walk(A, T, O.one(inst, s), int(seeds[s]), policy, mwt, switch=switch)
            r = LA.result(A, T, O.one(inst, s), w, mwt)
            O.assert_summary(sm[b], r, f"{name} {policy} env {b} <- {s} switch {switch}")
            if switch is None:
                own = O.episodes(A, T, O.one(inst, s), seeds[s], policy, 1, mwt)[0]
                assert r["reward"] == own["reward"] and r["n_steps"] == own["n_steps"]
    src.close(); dst.close()


# ---------------------------------------------------------------------------------------------------------------- 3. in place
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "g2x3", "wide"])
def test_in_place(gpu_device, name):
    env = destination(gpu_device, name)
    env.rollout("random", write_obs=False, max_decisions=np.arange(B_DST, dtype=np.int64) % 5)      # thirteen different states
    before = sections(env)
    # sources 0, 2, 5, 7, 10 and 12 are their own sources
    idx = np.array([0, 0, 2, 2, 2, 5, -1, 7, 7, 5, 10, 10, 12], np.int32)
    assert all(idx[s] == s for s in idx if s >= 0)
    rc, msg, ok = fork_raw(env, env, idx)
    assert rc == 0 and ok.tolist() == [1] * B_DST, (rc, msg, ok)
    moved = np.flatnonzero(idx >= 0)
    want = {k: v.copy() for k, v in before.items()}
    for k in want:
        want[k][moved] = before[k][idx[moved]]
    after = sections(env)
    assert_rows(after, want, slice(None), slice(None), "in place")
    # the copies kept their sources' seeds: three more decisions leave each equal to its source
    env.rollout("random", write_obs=False, max_decisions=3)
    cont = sections(env)
    assert_rows(cont, {k: v[idx[moved]] for k, v in cont.items()}, moved, slice(None), "continued in place")
    env.restore_state(blob_of(env, after))
    # new seeds: every env that has a source gets its own, also where s == b and nothing else may change
    new = np.arange(100, 100 + B_DST, dtype=np.uint64) << np.uint64(33)
    env.fork_from(env, idx, seeds=new, check=True)
    want["record"][moved, 8:16] = seed_bytes(new)[moved]
    seeded = sections(env)
    assert_rows(seeded, want, slice(None), slice(None), "in place, with seeds_in")
    # the refuse-and-skip path: env 1 names env 3, which is not its own source (3 <- 2); env 4 and env 6 leave the range.  The refused
    # envs are neither written nor read
    bad = idx.copy()
    bad[[1, 4, 6]] = [3, B_DST, -2]
    rc, msg, ok = fork_raw(env, env, bad, seeds=new + np.uint64(1))
    assert rc == 0 and ok.tolist() == [0 if b in (1, 4, 6) else 1 for b in range(B_DST)], (rc, msg, ok)
    taken = [b for b in moved if b not in (1, 4, 6)]
    want["record"][taken, 8:16] = seed_bytes(new + np.uint64(1))[taken]
    assert_rows(sections(env), want, slice(None), slice(None), "in place, refused envs untouched")
    from dcmrta_amd._lib import DcmError
    with pytest.raises(DcmError, match=r"3 env\(s\) were refused"):
        env.fork_from(env, bad, check=True)
    env.close()


@pytest.mark.gpu
def test_the_call_is_legal_under_stream_capture(gpu_device):
    """no host synchronisation: captured once, a replay copies what the source holds THEN"""
    import torch
    src, _ = source(gpu_device, "one")
    dst = destination(gpu_device, "one")
    idx = torch.from_numpy(MAP).to(dst.device)
    before = sections(dst)
    copied, alone = np.flatnonzero(MAP >= 0), np.flatnonzero(MAP < 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dst.fork_from(src, idx)
    src.rollout("random", write_obs=False, max_decisions=2)                    # the source moves on (the DONE env restarts)
    now = sections(src)
    g.replay()
    torch.cuda.synchronize()
    after = sections(dst)
    assert_rows(after, now, copied, MAP[copied], "replayed copy")
    assert_rows(after, before, alone, alone, "rows left alone")
    src.close(); dst.close()


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def refused(dst, src, index, code, *words, seeds=None):
    """the call is refused with `code` and a message that names the function and holds `words`; both handles keep their bytes"""
    keep = [(e, e.clone_state().cpu().numpy()) for e in {id(dst): dst, id(src): src}.values() if e is not None]
    rc, msg, ok = fork_raw(dst, src, index, seeds)
    assert rc == code and "dcm_fork_envs" in msg and all(w in msg for w in words), (rc, msg)
    assert ok.tolist() == [7] * dst.B, "nothing may be launched"
    for e, blob in keep:
        assert e.clone_state().cpu().numpy().tobytes() == blob.tobytes(), msg


@pytest.mark.gpu
def test_refusals_change_nothing(gpu_device):
    import torch
    from dcmrta_amd.batched_env import BatchedTaskEnv
    from dcmrta_amd.instances import generate_batch, generate_batch_ranges
    src, _ = source(gpu_device, "one")
    dst = destination(gpu_device, "one")
    A, T, mwt = 20, 50, 2.0

    def other(B, a=A, t=T, reset=True, load=True, **kw):
        e = BatchedTaskEnv(B, a, t, device=gpu_device, max_waiting_time=mwt, **kw)
        if load:
            e.load_instances(**generate_batch(B, a, t, base_seed=5))
            if reset:
                e.reset(3, observe=False)
        return e
    # DCM_ERR_INVALID: another record layout, a NULL map
    for e in (other(B_DST, a=21), other(B_DST, t=49), other(B_DST, member_cap=16)):
        refused(e, src, MAP, ERR_INVALID, "record layout")
        refused(dst, e, np.zeros(B_DST, np.int32), ERR_INVALID, "record layout")
        e.close()
    refused(dst, src, None, ERR_INVALID, "src_index")
    refused(dst, dst, None, ERR_INVALID, "src_index")
    if torch.cuda.device_count() > 1:
        far = BatchedTaskEnv(B_DST, A, T, device="cuda:1", max_waiting_time=mwt)
        refused(dst, far, MAP, ERR_INVALID, "different devices")
        far.close()
    # DCM_ERR_STATE: never loaded, loaded and never reset -- as the destination (although the call would fill it) and as the source
    for e in (other(B_DST, load=False), other(B_DST, reset=False)):
        refused(e, src, MAP, ERR_STATE, "dst", "loaded and reset")
        refused(dst, e, np.zeros(B_DST, np.int32), ERR_STATE, "src", "loaded and reset")
        e.close()
    # ... a ragged batch, loaded or generated
    rag = BatchedTaskEnv(B_DST, A, T, device=gpu_device, max_waiting_time=mwt)
    rag.load_instances(**generate_batch_ranges(range(40, 40 + B_DST), (10, 20), (20, 50)))
    rag.reset(3, observe=False)
    refused(rag, src, MAP, ERR_STATE, "dst", "ragged", "host copy")
    refused(dst, rag, np.zeros(B_DST, np.int32), ERR_STATE, "src", "ragged")
    refused(rag, rag, np.arange(B_DST, dtype=np.int32), ERR_STATE, "ragged")
    rag.close()
    # ... a renewal stride
    ren = BatchedTaskEnv(B_DST, A, T, device=gpu_device, max_waiting_time=mwt)
    ren.generate_instances(77)
    ren.reset(3, observe=False)
    ren.set_instance_renewal(B_DST)
    refused(ren, src, MAP, ERR_STATE, "dst", "renewal stride")
    refused(dst, ren, np.zeros(B_DST, np.int32), ERR_STATE, "src", "renewal stride")
    # with the stride cleared the call goes through, and the handle is no generated batch any more: renewal is refused from then on
    ren.set_instance_renewal(0)
    ren.fork_from(src, MAP, check=True)
    from dcmrta_amd._lib import DcmError
    with pytest.raises(DcmError, match="dcm_set_instance_renewal"):
        ren.set_instance_renewal(B_DST)
    ren.set_instance_renewal(0)
    for e in (ren, src, dst):
        e.close()


@pytest.mark.gpu
def test_a_destination_that_had_a_restart_image_steps_across_an_episode_end(gpu_device, oracle_lib):
    """An auto-resetting one-chunk handle keeps the records its reset produced as the restart image of its lockstep kernel.  After a
    fork that image is another instance's: the handle must restart the COPIED instance when dcm_step ends the episode."""
    import torch
    name, c = "one", CASES["one"]
    A, T, mwt = c["A"], c["T"], c["mwt"]
    inst, seeds = instances(name)
    src = make_env(gpu_device, name, B_SRC).load_instances(**inst)
    src.reset(seeds, observe=False)
    dinst, dseeds = instances(name, "dst")
    dst = make_env(gpu_device, name, B_DST, auto_reset=True).load_instances(**dinst)
    dst.reset(dseeds, observe=False)                       # (the image is taken here, of dst's own instances)
    idx = np.full(B_DST, -1, np.int32)
    idx[[0, 5]] = [1, 4]
    dst.fork_from(src, idx, check=True)
    rows = {0: 1, 5: 4}
    eps = {b: O.episodes(A, T, O.one(inst, s), seeds[s], "random", 2, mwt, record=True) for b, s in rows.items()}
    n1 = {b: eps[b][0]["n_steps"] for b in rows}
    obs = dst.observe()
    done_at = max(n1.values()) + 3
    for i in range(done_at):
        mask, leader = obs.mask.cpu().numpy().astype(np.uint8), obs.leader.cpu().numpy()
        act = first_free(mask)
        for b, s in rows.items():
            ep, j = (eps[b][0], i) if i < n1[b] else (eps[b][1], i - n1[b])
            if j < ep["n_steps"]:
                assert np.array_equal(mask[b], ep["mask"][j]) and leader[b] == ep["leader"][j], (b, i, "mask / leader")
                act[b] = H.host_random_action(mask[b], int(seeds[s]), i)
                assert act[b] == ep["action"][j], (b, i)
        obs = dst.step(torch.from_numpy(act).to(dst.device))
        for b in rows:
            if i + 1 == n1[b]:
                O.assert_summary(dst.summary().cpu().numpy()[b], eps[b][0], f"env {b} first episode")
                assert int(dst.episodes()[b]) == 1
    src.close(); dst.close()
