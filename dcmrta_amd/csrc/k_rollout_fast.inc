// k_rollout_fast.inc -- the kernel k_rollout_fast and all its forms (k_form.inc), compiled once per form: the plain, renewing and
// size-renewing ones by rollout_fast.hpp, the others by rollout_policy.hpp, rollout_log.hpp, rollout_explore.hpp and rollout_best.hpp.
// Logging forms: Fast<>::apply appends to the log where it commits the member lanes.  Lane a keeps agent a's running length in a
// register (FastLog): loaded once at the head, zeroed at a restart, written back once at the end -- nothing is loaded in the decision
// loop on the log's behalf.
// Epsilon-greedy forms: the explore words of 64 decisions are computed one per lane at the key refill (a third lane vector beside kv
// and kv2: one mix64, the high word kept); per decision one v_readlane, one scalar compare against explore_q32 and a wave-uniform
// choice between DCM_POLICY_RANDOM and the base policy in front of decide_logged's ONE apply.  With the log unset: cap 0, nothing
// stored, no length loaded or written back.
// Best-keeping form (rollout_best.hpp): the epsilon-greedy code, the log always set, plus keep_best behind a finished episode; the
// lengths it needs are the FastLog registers.  Nothing of it is in the decision loop.
#define KBASE rollout_fast
#define KPOLICY_FORMS 1
#include "k_form.inc"
template <int CA, int CT, bool RS, bool OBS, bool PRIO = false>
__global__ __launch_bounds__(WAVE, 4) void KNAME(int A, int T, int PA, int PT, KP P, unsigned char* state, int episodes,
                                                      float* agents_out, float* tasks_out, uint8_t* mask_out,
                                                      int64_t* steps_out, double* summary, uint16_t* ablog,
                                                      KSIZES, int64_t budget_all, const int64_t* budget_in,
                                                      unsigned char* gscr, double* retlog, int retcap KRENEW_PARAM KPOLICY_PARAM) {
    const int e = env_of_workgroup(), lane = threadIdx.x;
    int eA, eT;
    env_dims<CA, CT, RS>(sizes, e, A, T, eA, eT);
    using F = Fast<CA, CT, RS, OBS>;
    using SimT = typename F::SimT;
    SimT S{eA, eT, PA, PT, smem, nullptr};
    const Lay L = S.L();
    S.scr = SimT::SCR_IN_LDS ? smem + L.lds_rec() : gscr + (size_t)e * L.scratch_bytes();
    const int BA = S.BA(A), BT = S.BT(T);
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    typename SimT::XY xy;
    S.template load_record<true, false>(rec, lane, xy);
    S.set_ablog(ablog, e, BA, BT, lane);
    S.set_retlog(retlog, retcap, e, lane);
    WSYNC();
    HdrRegs h = load_hdr(smem);
    // (the launch asks for 512 bytes of LDS behind everything the general code uses: the removal path's compaction table)
    F f{S, (uint4*)(smem + (SimT::SCR_IN_LDS ? L.lds_bytes() : SimT::lds_image_bytes(L)))};
    f.init(lane);
    f.build_removal_table(lane);
#ifdef KEXPLORES
    // the env's rows of the log as in the logging form, or -- no log set -- a log of cap 0, to which apply<true> stores nothing
    const bool logged = lg.len != nullptr;
    FastLog fl{lg.task + (size_t)e * BA * lg.cap, lg.arrival + (size_t)e * BA * lg.cap, logged ? lg.cap : 0,
               (logged && f.inA) ? lg.len[(size_t)e * BA + f.la] : 0};
    // explore_q32 in [0, 2^32] against a 32-bit word: `always` (2^32) or an unsigned 32-bit compare, both on the scalar unit
    const bool x_all = (explore_q32 >> 32) != 0ull;
    const uint32_t x_q = (uint32_t)explore_q32;
#elif defined(DCM_LOG)
    // the env's rows of the log: wave-uniform bases, the lane's entry addressed by a 32-bit offset (dcm_set_rollout_log bounds A x cap)
    FastLog fl{lg.task + (size_t)e * BA * lg.cap, lg.arrival + (size_t)e * BA * lg.cap, lg.cap, f.inA ? lg.len[(size_t)e * BA + f.la] : 0};
#endif
    float* agrow = nullptr; float* tkrow = nullptr; uint8_t* mkp = nullptr;
    if constexpr (OBS) {
        float* ag = agents_out + (size_t)e * 6 * BA;
        float* tk = tasks_out + (size_t)e * 5 * (BT + 1);
        uint8_t* mk = mask_out + (size_t)e * (BT + 1);
        if constexpr (RS) S.write_pad_obs(lane, BA, BT, ag, tk, mk);
        agrow = ag + 6 * f.la;
        tkrow = tk + (f.inT ? 5 * (lane + 1) : 0);
        mkp = mk + (f.inT ? lane + 1 : 0);
    }
    double* row = summary + (size_t)e * 8;
    const int left0 = rollout_budget(e, budget_all, budget_in);
    int left = left0;
    uint64_t gd = h.seed + GAMMA * (h.d + 1);
    // the choice-protocol keys of the next 64 decisions, one per lane (25 VALU instructions per 64 decisions instead of a dependent
    // chain of 20 scalar ones at the head of every decision); ki = the lane that holds the current decision's key
    uint64_t kv = mix64(gd + GAMMA * (uint64_t)lane);
    uint64_t kv2 = mix64(kv + GAMMA);                  // ... and their second keys (follower draws 0 and 1)
#ifdef KEXPLORES
    uint32_t xv = (uint32_t)(mix64(kv ^ EXPLORE_SALT) >> 32);   // ... and their explore words
#endif
    int ki = 0;
    const uint64_t d0 = h.d;
    typename F::R r;
    f.load_consts(r);
    FPH_START(f);
    PH_DECL;
    int ep = 0;
    // the general event code has to run on the (flushed) LDS image before the next decision: a 0/1 word, pinned where the episode loop
    // tests it behind the decision loop -- as a bool it is a lane mask that the decision loop copies and inverts at its latch in every
    // trip.  (The epsilon-greedy and best-keeping forms keep the bool and the loop's three exits: with the word or with the one exit
    // they spill more SGPRs outside the loop, 113 VGPRs for 111.)
#ifdef KEXPLORES
    bool need_adv = 0;
#define NEED_ADV_PIN
#else
    int need_adv = 0;
#define NEED_ADV_PIN asm("" : "+s"(need_adv))
#endif
    // Wave priority = longest remaining work first (s_setprio).  A launch that fills the machine by itself ends with its slowest env
    // (430 of a mean 360 decisions at 20A/50T x 3 episodes) while the SIMDs it shares with envs that finished early idle; the waves
    // with the most tasks still to serve -- episodes to come x T + the unmasked tasks of the last decision, in sixths of the launch's
    // total: 4/6, 2/6, 1/6 -- win the instruction arbiter, so the four waves of a SIMD finish together: one 4096-env launch 1.237 ->
    // 1.091 ms (3 episodes), 0.447 -> 0.426 (1 episode), 8192 envs 2.23 -> 2.05.  Re-evaluated at episode ends and at the key refill
    // (every 64 decisions): nothing per decision.  Not for sub-batches that share the SIMDs with other launches (grid < 4096: several
    // streams, whose tails already overlap the others' bodies; priorities across launches measured -1 ... -5 % there, also with a
    // common deadline clock), nor in the multi-chunk kernels (their launches run in several rounds of workgroups: +0.5 / -3 %).
    // A template parameter, not a run-time test: the bookkeeping alone (one more live scalar, the refill path) cost the
    // unprioritised four-stream line 0.45 %.
    constexpr bool use_prio = PRIO;
    int nv_last = S.T(), prio_lv = 3;
    auto set_prio = [&](int ep_now) {
        const int rem6 = 6 * ((episodes - ep_now - 1) * S.T() + nv_last), tot = episodes * S.T();
        const int lv = rem6 >= 4 * tot ? 3 : (rem6 >= 2 * tot ? 2 : (rem6 >= tot ? 1 : 0));
        if (lv != prio_lv) {
            prio_lv = lv;
            if (lv == 3) __builtin_amdgcn_s_setprio(3); else if (lv == 2) __builtin_amdgcn_s_setprio(2);
            else if (lv == 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);
        }
    };
    if constexpr (use_prio) __builtin_amdgcn_s_setprio(3);
    for (;;) {
        if (need_adv == 0) {     // head of an episode slot (the `for ep` of k_rollout_random)
            if (ep >= episodes) break;
            if (h.flags & DCM_FLAG_DONE) {   // restart from the loaded instance; d keeps running
                if (h.flags & ROLLOUT_ERR) break;
                if (left == 0) break;        // budget spent at an episode boundary: the finished episode's results stay readable
#if DCM_RENEW == 2
                take_sizes(S, wave_renew_instance_sized_call(S, rec, rn, sizes, e, lane, xy));
                f.S.rA = S.rA; f.S.rT = S.rT;                                     // (Fast holds a copy of the simulator)
                f.init(lane);                                                     // lane ownership under the new sizes
                if constexpr (OBS) {
                    float* ag = agents_out + (size_t)e * 6 * BA;
                    float* tk = tasks_out + (size_t)e * 5 * (BT + 1);
                    uint8_t* mk = mask_out + (size_t)e * (BT + 1);
                    if constexpr (RS) S.write_pad_obs(lane, BA, BT, ag, tk, mk);  // rows between the new and the old sizes
                    agrow = ag + 6 * f.la;
                    tkrow = tk + (f.inT ? 5 * (lane + 1) : 0);
                    mkp = mk + (f.inT ? lane + 1 : 0);
                }
                if constexpr (use_prio) { nv_last = S.T(); set_prio(ep); }
#elif DCM_RENEW
                wave_renew_instance_call(S, rec, rn, e, lane, xy);
#endif
                S.reset_state(h, lane);
#if DCM_RENEW
                f.load_consts(r);
#endif
#if defined(DCM_LOG) || defined(KEXPLORES)
                fl.len = 0;                                                       // the log is the new episode's
#endif
                need_adv = 1;
            }
        }
        if (need_adv != 0) {
            CNT(15);
#if defined(KEXPLORES) || defined(DCM_POLICY)
            // The best-keeping form reads the row of every finished episode (keep_best).  The epsilon-greedy and greedy forms keep
            // terminal() because the rule below costs their decision loops: k_ex_ 1257 -> 1356 instructions, k_hp_ 1175 -> 1180.
            S.advance(h, P, lane, row PH_PASS);
#else
            // An episode that ends here with another one of this call to follow leaves a summary row nobody can read: the next
            // terminal() rewrites the row and the metrics' scratch, the restart clears the flags.  It takes the metric-free terminal
            // (flags, episode count, return log).  Not under a budget -- the next episode may stop half way, and the row must then
            // be the last FINISHED episode's -- and not for a flagged env, which stops at the restart.  Forms with the rule: plain,
            // renewing, logging and renewing-logging, each with compile-time sizes.
            // The runtime-size forms keep terminal(): with the second terminal in them their decision loops come out 1 - 3 instructions
            // longer and one of them a VGPR larger (tests/test_episode_boundary_host.py), so they compile to the code they had.
            if constexpr (RS) S.advance(h, P, lane, row PH_PASS);
            else {
                const bool no_metrics = left0 == NO_BUDGET && ep + 1 < episodes && !(h.flags & ROLLOUT_ERR);
                S.advance(h, P, lane, row PH_PASS, false, false, no_metrics);
#ifdef DCM_COUNT_PATHS
                if (h.flags & DCM_FLAG_DONE) { if (h.flags & SimT::FLAG_DEFERRED) CNT(19); else CNT(18); }
#endif
                h.flags &= ~SimT::FLAG_DEFERRED;                                  // internal: never stored, never seen by the loop
            }
#endif
            need_adv = 0;
            // wave-uniform by construction; tell the compiler so (scalar branches in the fast loop)
            h.now = uni(h.now); h.flags = uni(h.flags); h.cur_group = uni(h.cur_group); h.n_groups = uni(h.n_groups);
            h.empty_passes = uni(h.empty_passes);
        }
        if (!(h.flags & DCM_FLAG_DONE) && left != 0) {
            WSYNC();
            f.reload(r);
            FPHK(f, 13);
            for (;;) {
                FPHK(f, 12);
                CNT(0);
                const uint64_t k1 = rl(kv, ki);
                const Key2 k2{kv2, ki};                  // (the second key is read where the follower draws are: Fast<>::apply)
#ifdef KEXPLORES
                // the decision explores iff its explore word < explore_q32: then the random policy's action (protocol slot 1), else the base pick
                const bool explores = x_all || rl(xv, ki) < x_q;
                const int rlen = f.decide_logged(r, h, P, lane, k1, agrow, tkrow, mkp, &k2, explores ? DCM_POLICY_RANDOM : policy, fl);
#elif defined(DCM_LOG)
                const int rlen = f.decide_logged(r, h, P, lane, k1, agrow, tkrow, mkp, &k2, policy, fl);
#elif defined(DCM_POLICY)
                const int rlen = f.decide_policy(r, h, P, lane, k1, agrow, tkrow, mkp, &k2, policy);
#else
                const int rlen = f.decide(r, h, P, lane, k1, agrow, tkrow, mkp, &k2, use_prio ? &nv_last : nullptr);
#endif
#ifdef KEXPLORES
                if (h.flags & DCM_FLAG_DONE) break;
#else
                // ONE exit, at the foot, on `more` (the decisions left; 0 also for a finished episode and for an event that needs the
                // general code): with several exits the compiler gives the loop a lane mask per exit and merges them at the latch
                int more = 0;
                // (the flag bit as a number behind an opaque copy: `flags & 1` alone is a truncation to a bool, which the compiler
                //  branches on through a lane mask and vcc)
                uint32_t done = h.flags & DCM_FLAG_DONE;
                asm("" : "+s"(done));
                if (done == 0u) {
#endif
                gd += GAMMA;
#ifdef KEXPLORES
                if (++ki == WAVE) { kv = mix64(gd + GAMMA * (uint64_t)lane); kv2 = mix64(kv + GAMMA); xv = (uint32_t)(mix64(kv ^ EXPLORE_SALT) >> 32); ki = 0; }
#else
                if (++ki == WAVE) { kv = mix64(gd + GAMMA * (uint64_t)lane); kv2 = mix64(kv + GAMMA); ki = 0; if constexpr (use_prio) set_prio(ep); }
#endif
                left--;
                // worker.py:53 else same group, next leader.  The next-group step is an add, not a branch: as an arm of an
                // if / else-if beside next_event() it shared a latch block with the event, whose task_update / agent_update results
                // were then computed in shadow registers and copied back (11 v_mov behind every event, 8 of them 64-bit).
                // The latch's conditions are numbers on the scalar unit (common.hpp, the rule of the uniform conditions): `room`, the
                // groups still to come, and `turn` = room once the group is through, else 1 -- the next group if turn > 0 with the
                // group through, the next event if turn <= 0.  As bools (`rlen == 0`, `more_groups` and their three combinations) each
                // was a lane mask: 3 s_cselect_b64, 2 s_and / s_or_b64, a vcc formation and a vcc branch.
                const int room = h.n_groups - h.cur_group;
#ifdef DCM_COUNT_PATHS
                if (rlen == 0) { CNT(8); if (room > 0) CNT(9); }
#endif
                int turn = rlen == 0 ? room : 1, ahead = rlen == 0 ? room : 0;
                asm("" : "+s"(turn), "+s"(ahead));
                h.cur_group += (int)((0u - (uint32_t)ahead) >> 31);                 // worker.py:52 next group (1 iff ahead > 0: the sign of -ahead)
#ifdef KEXPLORES
                if (turn <= 0) {
                    if (!f.next_event(r, h, P, lane)) { need_adv = 1; break; }      // worker.py:85 -> :45
                }
                if (left == 0) break;
#else
                more = left;
                if (turn <= 0) {
                    if (!f.next_event(r, h, P, lane)) { need_adv = 1; more = 0; }   // worker.py:85 -> :45
                }
                }
                asm("" : "+s"(more));
                if (more == 0) break;
#endif
            }
            f.flush(r);
            FPHK(f, 12);
            NEED_ADV_PIN;
            if (need_adv != 0) continue;
        }
#ifdef DCM_BEST
        // a finished episode, its restart (fl.len = 0) still to come: keep it if it beats the kept one.  Also reached by an episode
        // that ends with the budget's last decision, which leaves the loop below without coming back.
        if ((h.flags & DCM_FLAG_DONE) && !(h.flags & ROLLOUT_ERR))
            keep_best<true>(best, lg, e, BA, S.A(), row, fl.len);
#endif
        if (left == 0) break;
        ep++;
        if constexpr (use_prio) { if (ep < episodes) { nv_last = S.T(); set_prio(ep); } }
    }
    PH_FLUSH(lane);
    FPHK(f, 13);
    FPH_FLUSH(f, lane);
#ifdef KEXPLORES
    if (logged && f.inA) lg.len[(size_t)e * BA + f.la] = fl.len;
#elif defined(DCM_LOG)
    if (f.inA) lg.len[(size_t)e * BA + f.la] = fl.len;
#endif
    const int64_t steps = (int64_t)(left0 - left);
    if (lane == 0 && steps_out) steps_out[e] = steps;
    h.d = d0 + (uint64_t)steps;
    {   // Hdr::max_arrival (see k_rollout_random)
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
#undef NEED_ADV_PIN
#include "k_form_end.inc"
