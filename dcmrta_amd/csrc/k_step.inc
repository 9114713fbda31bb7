// k_step.inc -- the kernel k_step and its forms k_rn_step and k_rs_step (k_form.inc), compiled once per form by dcmrta_env.hip
#define KBASE step
#include "k_form.inc"
template <int CA, int CT, bool RS, int MC = M>
__global__ __launch_bounds__(WAVE) void KNAME(int A, int T, int PA, int PT, KP P, unsigned char* state, const int32_t* actions,
                                              const int32_t* leader_in, const int32_t* nfol_in, const int16_t* fol_in,
                                              float* agents_out, float* tasks_out, uint8_t* mask_out,
                                              int32_t* leader_out, uint8_t* active_out, double* summary, RouteLog log,
                                              uint16_t* ablog, uint32_t mode, KSIZES, unsigned char* gscr,
                                              uint32_t max_episodes, double* retlog, int retcap KRENEW_PARAM) {
    const int e = env_of_workgroup(), lane = threadIdx.x;
    int eA, eT;
    env_dims<CA, CT, RS>(sizes, e, A, T, eA, eT);
    using SimT = Sim<CA, CT, RS, false, MC>;
    SimT S{eA, eT, PA, PT, smem, nullptr};
    using AMask = typename SimT::AMask;
    const Lay L = S.L();
    S.scr = gscr + (size_t)e * L.scratch_bytes();
    const int BA = S.BA(A), BT = S.BT(T);
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    PHK_DECL;
    // the host's per-env inputs are requested first, so that their memory latency hides behind the record copy instead of
    // being paid at their first use in the middle of the step (phase profile: ~1 us of every wave's critical path)
    const int act_in = actions[e];
    const int lead_in = leader_in ? leader_in[e] : -1;
    const int nf = nfol_in ? nfol_in[e] : -1;
        // (plain loads, not the non-temporal ones of the persistent kernel: with the record read AND rewritten every launch the
    //  default L2 policy measured 5.5 % faster at 65 536 envs, same at 4096)
    typename SimT::XY xy;
    S.template load_record<false>(rec, lane, xy);
    S.set_ablog(ablog, e, BA, BT, lane);
    S.set_retlog(retlog, retcap, e, lane);
    if (lane == 0) { *S.dirty() = 0; *S.dirty2() = 0; }
    WSYNC();
    HdrRegs h = load_hdr(smem);
    PHK_MARK(0);                                   // record HBM -> LDS (issue + wait)
    const bool was_active = !(h.flags & DCM_FLAG_DONE);
    if (was_active) {
        AMask gm;
        const uint64_t k1 = key1(h.seed, h.d);
        const int leader = S.pick_leader(h, lane, lead_in, k1, gm, (mode & DCM_PARAM_NO_GROUPING) != 0);
        PHK_MARK(1);                               // key + leader
        if (leader >= 0) {
            PH_DECL;
            S.apply_and_advance(h, P, lane, leader, gm, act_in, k1, nf,
                                fol_in ? fol_in + (size_t)e * DCM_FOLLOWER_COLS : nullptr, summary + (size_t)e * 8 PH_PASS,
                                log, e * BA, (mode & DCM_PARAM_NO_GROUPING) != 0, (mode & DCM_PARAM_STRICT_MASK) ? 2 : 1, false, true, &xy);
            PHK_MARK(2);                           // apply + updates + advance (+ terminal)
            PHK_INNER();
            // DCM_PARAM_AUTO_RESET: the episode has just ended (its results are in the summary row) -> start the next one from
            // the loaded instance, as k_rollout_random does between its episodes (the decision counter keeps running)
            if ((mode & DCM_PARAM_AUTO_RESET) && (h.flags & DCM_FLAG_DONE) &&
                !(h.flags & (DCM_FLAG_BAD_ACTION | DCM_FLAG_OVERFLOW | DCM_FLAG_BAD_LEADER | DCM_FLAG_BAD_INSTANCE)) &&
                (max_episodes == 0 || uni(((const Hdr*)smem)->episodes) < max_episodes)) {
#if DCM_RENEW == 2
                // (every row of the batch shape: agents beyond the new A read length 0 as well)
                if (log.len) for (int a = lane; a < BA; a += WAVE) log.len[(size_t)e * BA + a] = 0;
                take_sizes(S, wave_renew_instance_sized(S, rec, rn, sizes, e, lane, xy));   // the observation and its padding below: new sizes
#else
                if (log.len) for (int a = lane; a < eA; a += WAVE) log.len[(size_t)e * BA + a] = 0;
#if DCM_RENEW
                wave_renew_instance(S, rec, rn, e, lane, xy);
#endif
#endif
                S.reset_state(h, lane);
                if (lane == 0) *S.dirty() = SimT::DIRTY_ALL;
                S.advance(h, P, lane, summary + (size_t)e * 8 PH_PASS, (mode & DCM_PARAM_NO_GROUPING) != 0);
                PHK_MARK(3);                       // auto-reset: reset_state + first event
            }
        }
    }
    if (was_active) {
        WSYNC();
        store_hdr(h, lane);
        WSYNC();
        // Write back what this step can have changed: the header and the agent arrays always, status words always, and of
        // the other task sections only those marked dirty (one decision typically touches one member-arrival row, the id
        // word of one task and -- when a task became feasible -- the two time arrays: ~2.4 of the 4.6 KB at 20A/50T).
        // Ranges are widened to 16-byte boundaries; the bytes around them are unchanged copies of what HBM already holds.
        const uint32_t dm = uni(*S.dirty());
        const bool big = gridDim.x >= 8192u;           // far more state than the L2s hold: stream the stores (copy16_nt)
        auto put = [&](uint32_t lo, uint32_t hi) {     // [lo, hi) of the record
            lo &= ~15u; hi = (hi + 15u) & ~15u;
            if (big) copy16_nt(rec + lo, smem + lo, hi - lo, lane); else copy16(rec + lo, smem + lo, hi - lo, lane);
        };
        const uint32_t Tn = (uint32_t)S.PT();
        put(0, L.tb());                                                               // header + agent arrays
        const uint32_t d2 = uni(*S.dirty2());
        if ((dm & SimT::DIRTY_TIMES) && !(dm & SimT::DIRTY_NAB) && (d2 >> 24) == 1u) {   // one task became feasible: its pieces of the two arrays
            const uint32_t bt = d2 & 0xFFFFFFu;
            for (uint32_t sec : {L.ts(), L.tf()}) {
                const uint32_t lo = (sec + 8u * bt) & ~63u, end = sec + 8u * Tn;
                put(lo < sec ? sec : lo, lo + 64u < end ? lo + 64u : end);
            }
        } else if (dm & SimT::DIRTY_TIMES) put(L.ts(), L.marr());         // time_start, time_finish
        // a join (the only thing that dirties arrival rows / member ids without also dirtying the abandonment counts) names its
        // task: the aligned 64-byte pieces of those sections that hold it go back instead of the 8 T-byte sections
        const bool one_task = (dm & SimT::DIRTY_IDS) && !(dm & SimT::DIRTY_NAB) && (dm & SimT::DIRTY_ROWS) != SimT::DIRTY_ROWS;
        if (one_task) {
            const uint32_t jt = dm >> SimT::DIRTY_TASK_SHIFT;
            auto piece = [&](uint32_t sec) {
                const uint32_t lo = (sec + 8u * jt) & ~63u, end = sec + 8u * Tn;
                put(lo < sec ? sec : lo, lo + 64u < end ? lo + 64u : end);
            };
#pragma unroll
            for (int j = 0; j < MC; j++) if (dm & (2u << j)) piece(L.marr() + 8u * Tn * j);
            for (uint32_t w = 0; w < L.idw(); w++) piece(L.mids() + 8u * Tn * w);
        } else {
            if ((dm & SimT::DIRTY_ROWS) == SimT::DIRTY_ROWS) put(L.marr(), L.mids());
            else {
#pragma unroll
                for (int j = 0; j < MC; j++) if (dm & (2u << j)) put(L.marr() + 8u * Tn * j, L.marr() + 8u * Tn * (j + 1));
            }
            if (dm & SimT::DIRTY_IDS) put(L.mids(), L.tinfo());
        }
        put(L.tinfo(), (dm & SimT::DIRTY_NAB) ? L.mut_bytes() : L.tnab());  // status words (+ abandonment counts)
        PHK_MARK(5);                               // write-back (issue)
    }
    const bool want_obs = agents_out || tasks_out || mask_out || leader_out || active_out;
    if (want_obs) {
        WSYNC();
        float* ag = agents_out ? agents_out + (size_t)e * 6 * BA : nullptr;
        float* tk = tasks_out ? tasks_out + (size_t)e * 5 * (BT + 1) : nullptr;
        uint8_t* mk = mask_out ? mask_out + (size_t)e * (BT + 1) : nullptr;
        int leader = -1;
        if (!(h.flags & DCM_FLAG_DONE)) { AMask gm; leader = S.pick_leader(h, lane, -1, key1(h.seed, h.d), gm, (mode & DCM_PARAM_NO_GROUPING) != 0); }
        if (leader >= 0) {
            // The observation rows are built in LDS and leave as contiguous runs.  One lane per row writing its 5 or 6 floats
            // straight to HBM is a 20/24-byte-strided store (24 partial cache lines per wave instruction, 12 instructions);
            // staged, the same bytes are 6 fully coalesced instructions.  The staging area is the member-slot section of the
            // record image (arrival rows + id words): the write-back above has already read it, observe() never does, and
            // LDS operations of a wave execute in order -- so it costs no LDS (a separate 1.5 KB buffer would cost six
            // resident workgroups per CU, which is why round 2 measured staging slower).
            // Only for grids that fill the machine several times over (the HBM-bound regime: 165 -> 158 us at 65 536 envs);
            // a single round of workgroups is latency-bound and the extra LDS round trip costs it 0.8 us of 24 (4096 envs).
            const uint32_t need = 24u * (uint32_t)S.A() + 21u * ((uint32_t)S.T() + 1u) + 16u;
            if (gridDim.x >= 8192u && L.tinfo() - L.marr() >= need) {
                float* sag = (float*)(smem + L.marr());
                float* stk = sag + 6 * S.A();
                uint8_t* smk = (uint8_t*)(stk + 5 * (S.T() + 1));
                S.observe(h, lane, leader, ag ? sag : nullptr, tk ? stk : nullptr, mk ? smk : nullptr, xy);
                WSYNC();
                if (ag) for (int i = lane; i < 6 * S.A(); i += WAVE) __builtin_nontemporal_store(sag[i], ag + i);
                if (tk) for (int i = lane; i < 5 * (S.T() + 1); i += WAVE) __builtin_nontemporal_store(stk[i], tk + i);
                if (mk) for (int i = lane; i <= S.T(); i += WAVE) __builtin_nontemporal_store(smk[i], mk + i);
            } else {
                S.observe(h, lane, leader, ag, tk, mk, xy);
            }
        } else {
            S.write_inactive_obs(lane, ag, tk, mk);
        }
        if constexpr (RS || CA == 0) S.write_pad_obs(lane, BA, BT, ag, tk, mk);
        if (lane == 0) {
            if (leader_out) leader_out[e] = leader;
            if (active_out) active_out[e] = leader >= 0 ? 1 : 0;
        }
        PHK_MARK(4);                               // next leader + observation stores (issue)
    }
    PHK_TOTAL(6);
}
#include "k_form_end.inc"
