// k_rollout_fast_mc.inc -- the kernel k_rollout_fast_mc and its renewing form k_rn_rollout_fast_mc (k_form.inc), compiled once per
// form by rollout_fast_mc.hpp.  An exact shape, never ragged: no size-renewing form.
#define KBASE rollout_fast_mc
#include "k_form.inc"
template <int CA, int CT, bool OBS>
__global__ __launch_bounds__(WAVE, DCM_MC_WAVES) void KNAME(int A, int T, int PA, int PT, KP P, unsigned char* state, int episodes,
                                                         float* agents_out, float* tasks_out, uint8_t* mask_out,
                                                         int64_t* steps_out, double* summary, uint16_t* ablog,
                                                         const int32_t* sizes, int64_t budget_all, const int64_t* budget_in,
                                                         unsigned char* gscr, double* retlog, int retcap KRENEW_PARAM) {
    const int e = env_of_workgroup(), lane = threadIdx.x;
    using F = FastM<CA, CT, OBS>;
    using SimT = typename F::SimT;
    SimT S{CA, CT, PA, PT, smem, nullptr};
    constexpr Lay L{CA, CT};
    S.scr = gscr + (size_t)e * L.scratch_bytes();
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    S.gm = (double*)(rec + L.marr());
    typename SimT::XY xy;
    S.template load_record<true, false>(rec, lane, xy);
    S.set_ablog(ablog, e, CA, CT, lane);
    S.set_retlog(retlog, retcap, e, lane);
    if (lane == 0) S.inc_state()[1] = -1;
    WSYNC();
    HdrRegs h = load_hdr(smem);
    F f{S, rec};
    f.init(lane);
    float* ag = nullptr; float* tk = nullptr; uint8_t* mk = nullptr;
    if constexpr (OBS) {
        ag = agents_out + (size_t)e * 6 * CA;
        tk = tasks_out + (size_t)e * 5 * (CT + 1);
        mk = mask_out + (size_t)e * (CT + 1);
    }
    double* row = summary + (size_t)e * 8;
    const int left0 = rollout_budget(e, budget_all, budget_in);
    int left = left0;
    uint64_t gd = h.seed + GAMMA * (h.d + 1);
    const uint64_t d0 = h.d;
    typename F::R r;
    f.load_consts(r, xy, lane);
    PH_DECL;
    int ep = 0;
    bool need_adv = false;
    for (;;) {
        if (!need_adv) {         // head of an episode slot (the `for ep` of k_rollout_random)
            if (ep >= episodes) break;
            if (h.flags & DCM_FLAG_DONE) {
                if (h.flags & ROLLOUT_ERR) break;
                if (left == 0) break;
#if DCM_RENEW
                wave_renew_instance_call(S, rec, rn, e, lane, xy);
#endif
                S.reset_state(h, lane);
#if DCM_RENEW
                f.load_consts(r, xy, lane);
#endif
                need_adv = true;
            }
        }
        if (need_adv) {
            // no terminal metrics for an episode whose summary row the next one of this call rewrites (see k_rollout_fast.inc)
            const bool no_metrics = left0 == NO_BUDGET && ep + 1 < episodes && !(h.flags & ROLLOUT_ERR);
            S.advance(h, P, lane, row PH_PASS, false, false, no_metrics);
            h.flags &= ~SimT::FLAG_DEFERRED;
            need_adv = false;
            h.now = uni(h.now); h.flags = uni(h.flags); h.cur_group = uni(h.cur_group); h.n_groups = uni(h.n_groups);
            h.empty_passes = uni(h.empty_passes);
        }
        if (!(h.flags & DCM_FLAG_DONE) && left != 0) {
            WSYNC();
            f.reload(r, lane);
            for (;;) {
                const uint64_t k1 = mix64(gd);
                const int rlen = f.decide(r, h, P, lane, k1, ag, tk, mk);
                if (h.flags & DCM_FLAG_DONE) break;
                gd += GAMMA;
                left--;
                // worker.py:53 else same group, next leader; the next-group step branch-free (see k_rollout_fast.inc)
                const bool more_groups = h.cur_group < h.n_groups;
                h.cur_group += (rlen == 0 && more_groups) ? 1 : 0;                // worker.py:52 next group
                if (rlen == 0 && !more_groups) {
                    if (!f.next_event(r, h, P, lane)) { need_adv = true; break; }   // worker.py:85 -> :45
                }
                if (left == 0) break;
            }
            f.flush(r, lane);
            if (need_adv) continue;
        }
        if (left == 0) break;
        ep++;
    }
    PH_FLUSH(lane);
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
#include "k_form_end.inc"
