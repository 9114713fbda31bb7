// k_rollout_fast_g.inc -- the kernel k_rollout_fast_g and its forms k_rn_rollout_fast_g and k_rs_rollout_fast_g (k_form.inc),
// compiled once per form by rollout_fast_g.hpp
#define KBASE rollout_fast_g
#include "k_form.inc"
template <int NAC, int NTC, bool OBS>
__global__ __launch_bounds__(WAVE, DCM_G_WAVES) void KNAME(int A, int T, int PA, int PT, KP P, unsigned char* state, int episodes,
                                                        float* agents_out, float* tasks_out, uint8_t* mask_out,
                                                        int64_t* steps_out, double* summary, uint16_t* ablog,
                                                        KSIZES, int64_t budget_all, const int64_t* budget_in,
                                                        unsigned char* gscr, double* retlog, int retcap KRENEW_PARAM) {
    const int e = env_of_workgroup(), lane = threadIdx.x;
    int eA, eT;
    env_dims<128, 256, true>(sizes, e, A, T, eA, eT);
    using F = FastG<NAC, NTC, OBS>;
    using SimT = typename F::SimT;
    SimT S{eA, eT, PA, PT, smem, nullptr};
    const Lay L = S.L();
    S.scr = gscr + (size_t)e * L.scratch_bytes();
    unsigned char* rec = state + (size_t)e * L.rec_bytes();
    typename SimT::XY xy;
    S.template load_record<true, false>(rec, lane, xy);
    S.set_ablog(ablog, e, A, T, lane);
    S.set_retlog(retlog, retcap, e, lane);
    if (lane == 0) S.inc_state()[1] = -1;
    WSYNC();
    HdrRegs h = load_hdr(smem);
    // (the launch asks for 512 bytes of LDS behind everything the general code uses: the dummy slots)
    F f{S, (double*)(smem + SimT::lds_image_bytes(L))};
    f.init();
    float* ag = nullptr; float* tk = nullptr; uint8_t* mk = nullptr;
    if constexpr (OBS) {
        ag = agents_out + (size_t)e * 6 * A;
        tk = tasks_out + (size_t)e * 5 * (T + 1);
        mk = mask_out + (size_t)e * (T + 1);
        S.write_pad_obs(lane, A, T, ag, tk, mk);
    }
    double* row = summary + (size_t)e * 8;
    const int left0 = rollout_budget(e, budget_all, budget_in);
    int left = left0;
    uint64_t gd = h.seed + GAMMA * (h.d + 1);
    const uint64_t d0 = h.d;
    typename F::R r;
    f.load_consts(r, lane);
    PH_DECL;
    int ep = 0;
    bool need_adv = false;
    for (;;) {
        if (!need_adv) {         // head of an episode slot (the `for ep` of k_rollout_random)
            if (ep >= episodes) break;
            if (h.flags & DCM_FLAG_DONE) {
                if (h.flags & ROLLOUT_ERR) break;
                if (left == 0) break;
#if DCM_RENEW == 2
                take_sizes(S, wave_renew_instance_sized_call(S, rec, rn, sizes, e, lane, xy));
                f.S.rA = S.rA; f.S.rT = S.rT;                                     // (FastG holds a copy of the simulator; its lane masks,
                                                                                  //  chunk visits and wake-up times all read these two)
                if constexpr (OBS) S.write_pad_obs(lane, A, T, ag, tk, mk);       // rows between the new and the old sizes
#elif DCM_RENEW
                wave_renew_instance_call(S, rec, rn, e, lane, xy);
#endif
                S.reset_state(h, lane);
#if DCM_RENEW
                f.init();                                                         // the depot and the lanes' task constants
                f.load_consts(r, lane);
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
