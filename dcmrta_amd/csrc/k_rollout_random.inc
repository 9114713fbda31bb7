// k_rollout_random.inc -- the kernel k_rollout_random and all its forms (k_form.inc), compiled once per form: the plain, renewing and
// size-renewing ones by dcmrta_env.hip, the others by rollout_policy.hpp, rollout_log.hpp, rollout_explore.hpp, rollout_best.hpp,
// rollout_lookahead.hpp and rollout_individual.hpp.
// Logging forms: apply_and_advance appends to the log, and the env zeroes its lengths when it restarts an episode.
// Epsilon-greedy forms: a decision whose explore word (mix64(key_1 ^ EXPLORE_SALT) >> 32) is below explore_q32 takes
// pick_random_action, every other one pick_policy_action of the base policy (FIRST / NEAREST).  The budget is the greedy forms'
// (rollout_budget_policy).
// Best-keeping form (rollout_best.hpp): the epsilon-greedy decision with `policy` covering DCM_POLICY_RANDOM and the budget rule of the
// logging forms (explore_q32 = 0 there: the k_lg_* launch), plus keep_best behind the decision loop of a finished episode.
// Lookahead form (rollout_lookahead.hpp): the logging form's loop -- budget rule, restart, observation rows, log, all of them the OUTER
// decisions' -- with lookahead_action in the place of the policy's pick: the wave plays one inner episode per unmasked action
// between two snapshots of its env and takes the action whose episode ends best.  `width` limits the valued actions to the nearest
// ones (0: all of them), and `inner_out`, if set, takes the env's count of the inner episodes' decisions beside steps_out.
// Individual-selection form (rollout_individual.hpp): the epsilon-greedy loop with `policy` covering DCM_POLICY_RANDOM and the budget
// rule of the logging forms, and three call sites changed: pick_leader takes the lowest pending id (no draw), and apply_and_advance
// and both advance calls run with no_grouping -- no followers, the depot action moves the decider alone, ONE group per event.
#define KBASE rollout_random
#define KPOLICY_FORMS 1
#define KLOOKAHEAD_FORM 1
#define KINDIVIDUAL_FORM 1
#include "k_form.inc"
template <int CA, int CT, bool RS, int MC = M>
__global__ __launch_bounds__(WAVE, 3) void KNAME(int A, int T, int PA, int PT, KP P, unsigned char* state, int episodes,
                                                        float* agents_out, float* tasks_out, uint8_t* mask_out,
                                                        int64_t* steps_out, double* summary, uint16_t* ablog,
                                                        KSIZES, int64_t budget_all, const int64_t* budget_in,
                                                        unsigned char* gscr, double* retlog, int retcap KRENEW_PARAM KPOLICY_PARAM) {
    const int e = env_of_workgroup(), lane = threadIdx.x;
    int eA, eT;
    env_dims<CA, CT, RS>(sizes, e, A, T, eA, eT);
    using SimT = Sim<CA, CT, RS, (CT > WAVE) && !RS, MC>;   // member arrival times in the HBM record (MG) for the exact multi-chunk shapes
    SimT S{eA, eT, PA, PT, smem, nullptr};
    using AMask = typename SimT::AMask;
    const Lay L = S.L();
    S.scr = SimT::SCR_IN_LDS ? smem + L.lds_rec() : gscr + (size_t)e * L.scratch_bytes();
    const int BA = S.BA(A), BT = S.BT(T);
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    S.gm = (double*)(rec + L.marr());
    typename SimT::XY xy;
    S.template load_record<true, false>(rec, lane, xy);
    S.set_ablog(ablog, e, BA, BT, lane);
    S.set_retlog(retlog, retcap, e, lane);
    if (lane == 0) S.inc_state()[1] = -1;  // incremental task_update: nothing is known about the last call of the previous launch
    WSYNC();
    HdrRegs h = load_hdr(smem);
    float* ag = agents_out ? agents_out + (size_t)e * 6 * BA : nullptr;
    float* tk = tasks_out ? tasks_out + (size_t)e * 5 * (BT + 1) : nullptr;
    uint8_t* mk = mask_out ? mask_out + (size_t)e * (BT + 1) : nullptr;
    if constexpr (RS || CA == 0) S.write_pad_obs(lane, BA, BT, ag, tk, mk);
    // the usual call gives all three observation buffers: say so once, so that the per-decision null checks of observe() fold
    // (wave-uniform branches otherwise, at every decision)
    const bool all_obs = agents_out && tasks_out && mask_out;
    double* row = summary + (size_t)e * 8;
#if defined(DCM_POLICY) || defined(DCM_EXPLORE)
    const int left0 = rollout_budget_policy(e, budget_all, budget_in, P);
#elif defined(DCM_LOG) || defined(DCM_BEST) || defined(DCM_LOOKAHEAD) || defined(DCM_INDIVIDUAL)
    const int left0 = policy == DCM_POLICY_RANDOM ? rollout_budget(e, budget_all, budget_in) : rollout_budget_policy(e, budget_all, budget_in, P);
#else
    const int left0 = rollout_budget(e, budget_all, budget_in);
#endif
    int left = left0;
#ifdef DCM_LOOKAHEAD
    int64_t inner = 0;   // base-policy decisions inside inner episodes (wave-uniform): inner_out
#endif
    PH_DECL;
    // key_1 = mix64(seed + GAMMA (d+1)): the argument is carried and advanced by GAMMA per decision (no 64-bit multiply,
    // and neither seed nor d stay live in the loop: d = d0 + steps afterwards)
    uint64_t gd = h.seed + GAMMA * (h.d + 1);
    const uint64_t d0 = h.d;
    for (int ep = 0; ep < episodes; ep++) {
        if (h.flags & DCM_FLAG_DONE) {  // restart from the loaded instance; d keeps running
            if (h.flags & ROLLOUT_ERR) break;
            if (left == 0) break;       // budget spent at an episode boundary: the finished episode's results stay readable
#if DCM_RENEW == 2
            take_sizes(S, wave_renew_instance_sized_call(S, rec, rn, sizes, e, lane, xy));
            if constexpr (RS || CA == 0) S.write_pad_obs(lane, BA, BT, ag, tk, mk);   // rows between the new and the old sizes
#elif DCM_RENEW
            wave_renew_instance_call(S, rec, rn, e, lane, xy);
#endif
#if defined(KEXPLORES) || defined(DCM_LOOKAHEAD) || defined(DCM_INDIVIDUAL)
            if (lg.len) for (int a = lane; a < S.A(); a += WAVE) lg.len[(size_t)e * BA + a] = 0;   // the log, if set, is the new episode's
#elif defined(DCM_LOG)
            for (int a = lane; a < S.A(); a += WAVE) lg.len[(size_t)e * BA + a] = 0;   // the log is the new episode's (as k_step's restart)
#endif
            S.reset_state(h, lane);
#ifdef DCM_INDIVIDUAL
            S.advance(h, P, lane, row PH_PASS, true);   // every decider of the event in ONE group
#else
            S.advance(h, P, lane, row PH_PASS);
#endif
            PH_MARK(10);
        }
        // (the budget test rides on the loop's own scalar branch; testing it between observe and the action pick instead
        //  splits the hot block and was measured 2.3 % slower)
        while (!(h.flags & DCM_FLAG_DONE) && left != 0) {
            AMask gm;
            const uint64_t k1 = mix64(gd);   // (computing the next decision's key early, under the LDS latency of apply, measured
                                             //  0.9 % SLOWER: two more live registers across the whole decision)
#ifdef DCM_INDIVIDUAL
            const int leader = S.pick_leader(h, lane, -1, k1, gm, true);   // the lowest pending id: protocol slot 0 is not consumed
#else
            const int leader = S.pick_leader(h, lane, -1, k1, gm);
#endif
            if (leader < 0) break;
            PH_MARK(0);
            if (all_obs) { __builtin_assume(ag != nullptr); __builtin_assume(tk != nullptr); __builtin_assume(mk != nullptr); S.observe(h, lane, leader, ag, tk, mk, xy); }
            else S.observe(h, lane, leader, ag, tk, mk, xy);
            PH_MARK(1);
#ifdef KEXPLORES
            // the decision explores iff its explore word < explore_q32 (wave-uniform): protocol slot 1 then, the base policy's pick otherwise
            const bool explores = (uint64_t)(uint32_t)(mix64(k1 ^ EXPLORE_SALT) >> 32) < explore_q32;
#ifdef DCM_BEST
            const int action = (explores || policy == DCM_POLICY_RANDOM) ? S.pick_random_action(lane, k1) : S.pick_policy_action(lane, leader, policy, xy);
#else
            const int action = explores ? S.pick_random_action(lane, k1) : S.pick_policy_action(lane, leader, policy, xy);
#endif
#elif defined(DCM_INDIVIDUAL)
            // the epsilon-greedy decision, `policy` covering DCM_POLICY_RANDOM (explore_q32 = 0 there)
            const bool explores = (uint64_t)(uint32_t)(mix64(k1 ^ EXPLORE_SALT) >> 32) < explore_q32;
            const int action = (explores || policy == DCM_POLICY_RANDOM) ? S.pick_random_action(lane, k1) : S.pick_policy_action(lane, leader, policy, xy);
#elif defined(DCM_LOOKAHEAD)
            const int action = lookahead_action(S, h, P, lane, leader, gm, k1, gd, policy, xy, snap, e, BA, BT, width, inner PH_PASS);
#elif defined(DCM_POLICY)
            const int action = S.pick_policy_action(lane, leader, policy, xy);
#elif defined(DCM_LOG)
            const int action = policy == DCM_POLICY_RANDOM ? S.pick_random_action(lane, k1) : S.pick_policy_action(lane, leader, policy, xy);
#else
            const int action = S.pick_random_action(lane, k1);
#endif
            PH_MARK(2);
#ifdef DCM_INDIVIDUAL
            // no_grouping: no followers and no follower draws, action 0 moves `leader` alone, and the next event is one group again
            S.template apply_and_advance<true>(h, P, lane, leader, gm, action, k1, -1, nullptr, row PH_PASS, lg, e * BA, true, 0, true, false, &xy);
#elif defined(DCM_LOG) || defined(KEXPLORES) || defined(DCM_LOOKAHEAD)
            S.template apply_and_advance<true>(h, P, lane, leader, gm, action, k1, -1, nullptr, row PH_PASS, lg, e * BA, false, 0, true, false, &xy);
#else
            S.template apply_and_advance<true>(h, P, lane, leader, gm, action, k1, -1, nullptr, row PH_PASS, RouteLog{nullptr, nullptr, nullptr, 0}, 0, false, 0, true, false, &xy);
#endif
            gd += GAMMA;
            left--;
        }
#ifdef DCM_BEST
        // a finished episode, its restart (the lg.len zeroing) still to come: keep it if it beats the kept one
        if ((h.flags & DCM_FLAG_DONE) && !(h.flags & ROLLOUT_ERR))
            keep_best<false>(best, lg, e, BA, S.A(), row, 0);
#endif
        if (left == 0) break;
    }
    PH_FLUSH(lane);
    const int64_t steps = (int64_t)(left0 - left);
    if (lane == 0 && steps_out) steps_out[e] = steps;
#ifdef DCM_LOOKAHEAD
    if (lane == 0 && inner_out) inner_out[e] = inner;
#endif
    h.d = d0 + (uint64_t)steps;   // every decision of this kernel is valid, so apply_and_advance counted exactly `steps`
    {   // Hdr::max_arrival: this kernel only takes valid actions, under which every arrival list is monotone, so the maximum of
        // the agents' last arrivals IS the running maximum of the episode so far -- folded in once per launch for a later
        // dcm_step on the same episode
        double m = 0.0;
        S.for_agents(lane, [&](int a) { const double av = (S.cur()[a] != -2) ? S.arr()[a] : 0.0; m = av > m ? av : m; });
        const double wm = wave_nanmax(m);
        if (lane == 0) { Hdr* q = (Hdr*)smem; if (wm > q->max_arrival) q->max_arrival = wm; }
    }
    WSYNC();
    store_hdr(h, lane);
    WSYNC();
    S.store_record(rec, lane);
}
#include "k_form_end.inc"
