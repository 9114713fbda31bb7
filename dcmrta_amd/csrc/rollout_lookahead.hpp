// rollout_lookahead.hpp -- the lookahead form of the persistent rollout (dcm_rollout_lookahead): every decision of every env is chosen
// by one-step lookahead over a base policy (DCM_POLICY_RANDOM / FIRST / NEAREST) -- the rollout algorithm, Lookahead.values() +
// best_actions() of dcmrta_amd/lookahead.py -- inside ONE persistent launch and without a branch handle.
// Included by dcmrta_env.hip inside its anonymous namespace, after rollout_fast.hpp, in the translation unit of this form only
// (-DDCM_TU_A, or a one-unit developer build).
//
// The form is the general kernel text compiled once more:
//   k_la_rollout_random / k_larn_rollout_random  from k_rollout_random.inc  every launch
// with the logging forms' arguments (`policy`: the BASE policy; the log may be unset, lg.len null) plus `snap`, the handle's snapshot
// buffer.  One wave owns one env, and that wave values its own actions one after the other (lookahead_action below), so nothing is
// synchronised across workgroups and nothing returns to the host.  k_larn_* renews a uniform generated batch's instances at (outer)
// episode restarts like k_rn_*.  No size-renewing form (the host refuses that launch), no wave-priority instantiation, and no form
// of k_rollout_fast, k_rollout_fast_mc or k_rollout_fast_g: every shape takes k_la_rollout_random.
//
// The snapshot lives in HBM, the env's slice of a handle-owned buffer laid out like one env of the dcm_clone_state blob: the record
// image (store_record's), 64 B (the summary row's place, unused: the inner episodes never write the row), the env's rows of the
// abandonment log and its overflow count table.  A second LDS copy of the record is the alternative; NOBODY HAS MEASURED the choice.
// HBM was taken because it keeps the LDS request, and with it the resident workgroups per CU, of the general kernel, and because
// the side rows live in HBM anyway; the restore after an inner episode (4.5 KB at 20A/50T) follows some hundred decisions.
#pragma once

// The action decision d takes under the lookahead rule.  The env sits in front of decision d (leader and group mask drawn, key_1 =
// k1 = mix64(gd)).  For every unmasked task t, ascending:
//   1. decision d takes action t + 1 with this leader and the followers of slots 2+j of k1, as the real step will;
//   2. the base policy plays decisions d+1, d+2, ... (keys mix64(gd + GAMMA), ...) until the episode ends -- apply_and_advance<DEV, INNER>:
//      no observation rows, no log, and terminal_inner in the place of terminal(): no metrics, no summary row, no episode count, no
//      return log;
//   3. its value is (finished tasks, -now) of the state the episode ended in: entries 1 and 0 of the summary row terminal() would
//      have written -- also for an inner episode that ends TRUNCATED (the zero-decider guard) or at max_time, which is what
//      Lookahead.values() reads from such a branch's row; an inner episode that stops under an error flag (pick_leader's BAD_LEADER,
//      unreachable: groups are never empty) is valued by the state it stopped in, where the host-driven form would read the row of
//      an earlier episode -- the one case in which the two could differ, and not reachable with the device's own valid actions;
//   4. the env is put back: overflow counts, abandonment rows, record image (and, MG, the member arrival times in the HBM record);
//      the incremental task_update is told that it knows nothing of the previous call, as at the head of a launch.
// The best value wins -- more finished tasks, then the larger reward, exact in fp64, and a tie goes to the lowest action index.
// No unmasked task: the depot (0), the one allowed action; exactly one: that task; neither costs a snapshot or an inner episode.
// `width` (dcm_rollout_lookahead_width; 0 = every unmasked task, the rule above) values only the `width` unmasked tasks NEAREST would
// pick one after the other if each pick were masked for the next: the `width` smallest by (rounded fp64 dist2 from the leader, task
// index).  T goes up to 1023, so the list is never stored: after every inner episode the env is back bit for bit, mask and distances
// included, and Sim::next_nearest_task finds the next candidate behind a wave-uniform cursor (the last one's distance and index).
// The candidates are valued in that order, hence the explicit index tie-break of the best-pair compare; width >= the number of
// unmasked tasks takes the ascending loop of width 0, inner episode for inner episode; width == 1 is NEAREST's pick itself, with no
// snapshot and no inner episode, whatever the base policy.
// `inner` counts the base-policy decisions of the inner episodes: every apply_and_advance<true, true> below but each episode's first,
// which is decision d itself (wave-uniform; the kernel stores it to inner_out once, at its end).
// `h`, the hot header fields, is copied for the inner episodes and never changed; the cold ones travel with the record image.
// The overflow count table is only ever touched by an agent's 17th abandonment of an episode, and is all zero while no agent has
// had one (Sim::clear_spilled_counts): it is saved only if the env has spilled when the snapshot is taken, and after an inner
// episode that spilled it is copied back or, if nothing was saved, zeroed.
template <class SimT>
__device__ __forceinline__ int lookahead_action(const SimT& S, const HdrRegs& h, const KP& P, int lane, int leader,
                                                const typename SimT::AMask& gm, uint64_t k1, uint64_t gd, int policy,
                                                const typename SimT::XY& xy, unsigned char* snap, int e, int BA, int BT, int width,
                                                int64_t& inner PH_ARGS) {
    const int T_ = S.T();
    auto unmasked = [](uint32_t info) { return !(info & T_FEAS) && ((int)(int8_t)((info >> 8) & 0xFF) > 0); };   // :199, as observe()
    int nfree = 0, lowest = -1;
    for (int t0 = 0; t0 < T_; t0 += WAVE) {
        const int t = t0 + lane;
        const uint64_t bm = __ballot((t < T_) && unmasked(S.tinfo()[t < T_ ? t : 0]));
        if (bm && lowest < 0) lowest = t0 + __ffsll((unsigned long long)bm) - 1;
        nfree += __popcll(bm);
    }
    if (nfree == 0) return 0;
    if (nfree == 1) return lowest + 1;
    if (width == 1) return S.pick_policy_action(lane, leader, DCM_POLICY_NEAREST, xy);
    const bool all = width == 0 || width >= nfree;   // wave-uniform

    const Lay L = S.L();
    unsigned char* const img = snap + (size_t)e * ((size_t)L.rec_bytes() + 64u + 32u * (size_t)BA + abcnt_pitch(BA, BT));
    unsigned char* const rows = img + L.rec_bytes() + 64;
    unsigned char* const cnts = rows + 32 * (size_t)BA;
    const uint32_t row_bytes = 2u * AB_CAP * (uint32_t)S.A(), cnt_bytes = (uint32_t)abcnt_pitch(S.A(), T_);
    auto spilled = [&]() {
        bool sp = false;
        S.for_agents(lane, [&](int a) { sp = sp || (S.ainfo()[a] >> 16) > (uint32_t)AB_CAP; });
        return __any(sp) != 0;
    };
    WSYNC();
    const bool spilled0 = spilled();
    S.store_record(img, lane);
    S.snapshot_marr(img, lane);
    copy16_in(rows, (const unsigned char*)S.ablog(), row_bytes, lane);
    if (spilled0) copy16_in(cnts, (const unsigned char*)S.abcnt(), cnt_bytes, lane);

    int best = 0;
    double bn = -1.0, br = 0.0;
    double pd = -1.0;   // the candidate cursor: in front of every task
    for (int t = lowest - 1, n = 0;; n++) {
        if (all) {
            do t++; while (t < T_ && !unmasked(uni(S.tinfo()[t])));
            if (t >= T_) break;
        } else {
            if (n == width) break;
            t = S.next_nearest_task(lane, leader, pd, t, xy, pd);   // n < width < nfree: there is one
        }
        HdrRegs hi = h;
        uint64_t gi = gd, k = k1;
        int ld = leader, act = t + 1;
        typename SimT::AMask g2 = gm;
        for (;;) {
            S.template apply_and_advance<true, true>(hi, P, lane, ld, g2, act, k, -1, nullptr, nullptr PH_PASS,
                                                     RouteLog{nullptr, nullptr, nullptr, 0}, 0, false, 0, true, false, &xy);
            gi += GAMMA;
            if (hi.flags & DCM_FLAG_DONE) break;
            k = mix64(gi);
            ld = S.pick_leader(hi, lane, -1, k, g2);
            if (ld < 0) break;
            act = policy == DCM_POLICY_RANDOM ? S.pick_random_action(lane, k) : S.pick_policy_action(lane, ld, policy, xy);
            inner++;
        }
        WSYNC();
        int nfin = 0;
        for (int t0 = 0; t0 < T_; t0 += WAVE) {
            const int u = t0 + lane;
            nfin += __popcll(__ballot(u < T_ && (S.tinfo()[u < T_ ? u : 0] & T_FIN)));
        }
        const double cn = (double)nfin, cr = -hi.now;
        // (one predicate and three selects, no branches: written as `if (cn > bn || (cn == bn && (...))) { best = ...; bn = cn; br = cr; }`
        //  hipcc 7 structurises the nested short-circuit over these VGPR-held doubles so that the cn == bn arm keeps the OLD br)
        const bool better = (cn > bn) | ((cn == bn) & ((cr > br) | ((cr == br) & (t + 1 < best))));
        best = better ? t + 1 : best;
        bn = better ? cn : bn;
        br = better ? cr : br;
        // put the env back
        const bool spilled1 = spilled();
        WSYNC();
        if (spilled1) {
            if (spilled0) copy16_in((unsigned char*)S.abcnt(), cnts, cnt_bytes, lane);
            else { uint4* c = (uint4*)S.abcnt(); for (uint32_t i = lane; i < cnt_bytes / 16; i += WAVE) c[i] = uint4{0u, 0u, 0u, 0u}; }
        }
        copy16_in((unsigned char*)S.ablog(), rows, row_bytes, lane);
        S.load_mutable(img, lane);
        S.restore_marr(img, lane);
        if constexpr (SimT::INC) { if (lane == 0) S.inc_state()[1] = -1; }
        WSYNC();
    }
    return best;
}

#define DCM_LOOKAHEAD 1
#define DCM_RENEW 0
#include "k_rollout_random.inc"
#undef DCM_RENEW
#define DCM_RENEW 1
#include "k_rollout_random.inc"
#undef DCM_RENEW
#undef DCM_LOOKAHEAD
