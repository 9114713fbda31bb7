"""The epsilon-greedy device policies against the oracle (test infrastructure): consecutive episodes of one env under
rollout(base, explore_q32=q32), walked through the oracle's step-wise API (lookahead_ref.walk) with the definition's pick -- decision d
takes the random policy's action where choice.explores(seed, d, q32) says so and the base policy's pick otherwise -- and replayed by
the oracle's own rollout with the walk's choices injected, which gives the terminal results and the route lists."""
import lookahead_policy_ref as LP
import lookahead_ref as LA


def explore_episodes(a, t, inst_one, seed, base, q32, n, mwt=10.0, max_time=LA.MAX_TIME):
    """n consecutive episodes, the decision counter running on across them (a running counter is a seed shift: LP.shifted_seed).
    Per episode dict(n_steps, explored: decisions that took the random action, result: the oracle's terminal results, o: the OracleEnv
    of the replay (route lists), flags: the env's header after it, a)."""
    from dcmrta_amd.choice import explores
    out, d0 = [], 0
    for _ in range(n):
        s = LP.shifted_seed(seed, d0)
        explored = []

        def action_of(c):
            ex = explores(s, c.d, q32)
            explored.append(ex)
            return LA.base_pick("random" if ex else base, c.seed_of)(c.mask, c.pos, c.task_xy, c.d)

        w = LA.walk(a, t, inst_one, s, action_of, mwt, max_time=max_time)
        assert w["ended"]
        o, r, flags = LP.replay(a, t, inst_one, w, mwt, max_time)
        out.append(dict(n_steps=w["n_steps"], explored=sum(explored), result=r, o=o, flags=flags, a=a))
        d0 += w["n_steps"]
    return out
