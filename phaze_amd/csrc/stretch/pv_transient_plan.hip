// pv_transient_plan.hip -- pv_onsets_from_strength and pv_transient_plan of include/phaze_amd.h: from onset counts to onset positions, and from
// onset positions to the hop row and reset row of pv_transient_process.  Pure host code: no handle, no device.  The rules are DESIGN.md "Phase
// resets"; tests/transient_model.py restates them in numpy and tests/test_transient_abi.py compares the two exactly.
#include <stdint.h>

#include <algorithm>

#include "../../../include/phaze_amd.h"

extern "C" {

int64_t pv_onsets_from_strength(const int32_t *counts, int64_t nframes, int32_t fft_size, int32_t analysis_hop, double tau, int64_t *onsets, int64_t capacity)
{
    if (nframes < 0 || (nframes > 0 && !counts) || fft_size < 4 || analysis_hop < 1 || !(tau > 0.0) || capacity < 0 || (capacity > 0 && !onsets)) return -PV_ERR_ARGUMENT;
    const double thr = tau * (double)(fft_size / 2 - 1);               // tau (H - 2), H = N/2 + 1
    int64_t n = 0;
    bool above = false;                                                 // frame -1 is silent: below any tau > 0
    for (int64_t m = 0; m < nframes; m++) {
        const bool now = (double)counts[m] >= thr;
        if (now && !above) {
            if (n < capacity) onsets[n] = m * analysis_hop;
            n++;
        }
        above = now;
    }
    return n;
}

int64_t pv_transient_plan(const int64_t *onsets, int64_t nonsets, int64_t input_len, int32_t fft_size, int32_t nominal_hop, int32_t floor_hop,
                          int32_t synthesis_hop, int32_t lead, int32_t release, int32_t *hops, uint8_t *resets, int64_t capacity)
{
    const int64_t N = fft_size, ha = nominal_hop, fl = floor_hop, hs = synthesis_hop;
    if (N < 2 || (N & (N - 1)) != 0 || fl < 1 || ha < fl || ha > N || hs < 1 || hs > N / 2 || input_len < 0 || nonsets < 0 || (nonsets > 0 && !onsets)
        || capacity < 0 || (capacity > 0 && (!hops || !resets)))
        return -PV_ERR_ARGUMENT;
    if (hs < fl) return -PV_ERR_ARGUMENT;                               // a hold needs hop = hs to be a legal hop
    const int64_t L = lead < 0 ? N / 8 : lead;
    if (L > N / 2) return -PV_ERR_ARGUMENT;
    const int64_t rel = release < 0 ? N / 2 : release;                   // how long an attack is taken to last behind its position
    if (rel > N) return -PV_ERR_ARGUMENT;
    for (int64_t i = 1; i < nonsets; i++)
        if (onsets[i] < onsets[i - 1]) return -PV_ERR_ARGUMENT;
    const int64_t kappa = ha / 8 > 1 ? ha / 8 : 1;
    int64_t S = 0, m = 0;                                               // input consumed, frames planned
    bool held_prev = false;
    for (;;) {
        const int64_t tried = held_prev ? hs : ha;
        const int64_t lo = S + tried - N + L, hi = S + tried - L;       // the part [L, N - L) of the window that ends at S + tried
        const int64_t i = std::lower_bound(onsets, onsets + nonsets, lo - rel) - onsets;   // [onset, onset + release] meets [lo, hi)
        const bool held = i < nonsets && onsets[i] < hi;
        int64_t hop;
        if (held) {
            hop = hs;
        } else {
            int64_t debt = S - m * ha;
            if (debt > kappa) debt = kappa;
            if (debt < -kappa) debt = -kappa;
            hop = ha - debt;
            if (hop < fl) hop = fl;
            if (hop > N) hop = N;
        }
        if (S + hop > input_len) break;
        if (m < capacity) {
            hops[m] = (int32_t)hop;
            resets[m] = held && !held_prev ? 1 : 0;
        }
        S += hop;
        m++;
        held_prev = held;
    }
    return m;
}

}  // extern "C"
