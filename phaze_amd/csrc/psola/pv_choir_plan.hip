// pv_choir_plan.hip -- pv_choir_plan of include/phaze_amd.h: pv_tsm_plan with the time direction and the step of every grain.  Pure host code: no handle,
// no device.  The rules are DESIGN.md "Choir"; tests/choir_model.py restates them in Python and tests/test_choir_abi.py compares the two exactly, so the
// arithmetic below is written one operation at a time: no contraction.  The walk is pv_tsm_plan.hip's word for word (that file is pinned by its own tests
// and stays as it is); the direction, D and phi of a reuse are pv_mirror_plan's rule and the step and the half length pv_formant_plan's, restated here:
// with warps == NULL the grains are pv_mirror_plan's bits, with mirror == 0 pv_formant_plan's.
#include <math.h>
#include <stdint.h>

#include "../../../include/phaze_amd.h"
#include "pv_choir.h"

#pragma clang fp contract(off)

namespace {

int64_t floor_div(int64_t a, int64_t b)                                 // b > 0
{
    const int64_t q = a / b;
    return a % b < 0 ? q - 1 : q;
}

struct Track {
    const pv_psola_params *p;
    const pv_epoch_params *e;
    const int32_t *records;
    const double *ratios;
    const double *rates;
    const double *warps;
    const int32_t *epochs;
    int64_t nrec;
    // the record of position tau (pv_tune_plan's lookup at shift 0, on floor(tau)); -1 without records
    int64_t rec(double tau) const
    {
        if (nrec <= 0) return -1;
        int64_t j = floor_div((int64_t)floor(tau) - p->f0_center + p->f0_hop / 2, p->f0_hop);
        if (j < 0) j = 0;
        if (j > nrec - 1) j = nrec - 1;
        return j;
    }
    bool voiced(double tau) const
    {
        const int64_t j = rec(tau);
        return j >= 0 && pv_f0_period(records + 4 * j) > 0.0;
    }
    double period(double tau) const
    {
        const int64_t j = rec(tau);
        const double q = j >= 0 ? pv_f0_period(records + 4 * j) : 0.0;
        if (!(q > 0.0)) return p->unvoiced_period;
        if (q < (double)p->min_period) return (double)p->min_period;
        if (q > (double)p->max_period) return (double)p->max_period;
        return q;
    }
    double ratio(double tau) const
    {
        const int64_t j = rec(tau);
        if (j < 0 || !ratios || !(pv_f0_period(records + 4 * j) > 0.0)) return 1.0;
        return ratios[j];
    }
    // input samples consumed per output sample, held within [1/4, 4], voiced or not
    double rate(double tau) const
    {
        const int64_t j = rec(tau);
        if (j < 0 || !rates) return 1.0;
        const double r = rates[j];
        return r < 0.25 ? 0.25 : (r > 4.0 ? 4.0 : r);
    }
    // the step of the grain held for the analysis mark tau in 1/256, voiced or not: consonants move with the vowels
    int64_t warp(double tau) const
    {
        const int64_t j = rec(tau);
        if (j < 0 || !warps) return PV_TSM_Q;
        return (int64_t)floor(256.0 * warps[j] + 0.5);
    }
    // the largest distance between two synthesis marks: two grains of the longest half length still cover everything between their centres
    double cap() const { return p->max_period > 2 ? (double)(2 * p->max_period - 4) : 1.0; }
    // the distance to the next synthesis mark: period / ratio, at most cap()
    double step(double tau) const
    {
        const double s = period(tau) / ratio(tau);
        return s < cap() ? s : cap();
    }
    // pv_epoch_plan.hip's snap
    double snap(double c, const double *prev) const
    {
        const int64_t j = rec(c);
        if (!epochs || j < 0 || !(pv_f0_period(records + 4 * j) > 0.0) || epochs[4 * j + 1] <= 0 || epochs[4 * j + 3] < e->min_strength) return c;
        const double P = period(c);
        const double E = (double)(j * (int64_t)p->f0_hop + (int64_t)epochs[4 * j]);
        double s = E + floor((c - E) / P + 0.5) * P;
        if (prev && s - *prev < P / 2.0) s = s + P;
        if (prev && voiced(*prev) && fabs(s - c) <= P / 4.0) s = c + e->lock * (s - c);
        return s;
    }
};

}  // namespace

extern "C" {

int64_t pv_choir_plan(const pv_psola_params *p, const pv_epoch_params *e, const int32_t *records, int64_t nrec, const double *ratios, const double *rates,
                      const double *warps, const int32_t *epochs, int32_t mirror, int32_t *grains, int64_t capacity, int64_t *output_len)
{
    if (!p || p->struct_size != (int32_t)sizeof(pv_psola_params) || nrec < 0 || (nrec > 0 && !records) || capacity < 0 || (capacity > 0 && !grains))
        return -PV_ERR_ARGUMENT;
    if (!e || e->struct_size != (int32_t)sizeof(pv_epoch_params) || e->min_strength < 0 || e->min_strength > 16384 || !(e->lock > 0.0 && e->lock <= 1.0))
        return -PV_ERR_ARGUMENT;
    if (p->f0_hop < 1 || p->min_period < 2 || p->max_period < p->min_period || p->max_period > PV_TSM_MAX_PERIOD || p->reserved != 0
        || !(p->unvoiced_period >= (double)p->min_period && p->unvoiced_period <= (double)p->max_period) || p->input_len < 0
        || p->input_len >= PV_TSM_MAX_POSITION)
        return -PV_ERR_ARGUMENT;
    if (mirror != 0 && mirror != 1) return -PV_ERR_ARGUMENT;
    if (ratios)
        for (int64_t j = 0; j < nrec; j++)
            if (!(ratios[j] >= 0.5 && ratios[j] <= 2.0)) return -PV_ERR_ARGUMENT;
    if (rates)
        for (int64_t j = 0; j < nrec; j++)
            if (!(rates[j] > 0.0 && rates[j] < INFINITY)) return -PV_ERR_ARGUMENT;
    if (warps)
        for (int64_t j = 0; j < nrec; j++)
            if (!(warps[j] >= 0.5 && warps[j] <= 2.0)) return -PV_ERR_ARGUMENT;
    const Track tr{p, e, records, ratios, rates, warps, epochs, nrec};
    const double len = (double)p->input_len, far = tr.cap();
    double A = tr.snap(0.0, nullptr), An = tr.snap(A + tr.period(A), &A);   // the analysis mark in hand and the one after it
    double T = 0.0, Tprev = 0.0, V = 0.0, Vprev = 0.0;
    int64_t m = 0;
    bool past = false;                                                  // a centre at or beyond 2^30, or a mirrored D beyond int32: the table cannot say it
    // one grain is held back until the mark after it is final: its half length covers half the way to either neighbour
    bool held = false, hmir = false;
    double hT = 0.0, hA = 0.0, hV = 0.0, hgap = 0.0;
    const auto emit = [&](double gap_after) {
        // the grain reads s / 256 input samples per output sample, in either direction, so period 256 / s outputs cover one period of the input;
        // s = 256 divides by 1.0: exact
        const int64_t s = tr.warp(hA);
        double L = floor(tr.period(hA) / ((double)s / 256.0) + 0.5);
        const double g = hgap > gap_after ? hgap : gap_after, need = floor(g / 2.0) + 2.0;
        if (L < need) L = need;
        if (L < 2.0) L = 2.0;
        if (L > (double)p->max_period) L = (double)p->max_period;
        const int64_t c = (int64_t)floor(256.0 * hT + 0.5);
        if ((c >> 8) >= PV_TSM_MAX_POSITION) past = true;
        int64_t w, D;
        if (hmir) {                                                     // about its own mark: input hA - (s / 256) (tau - hT) lands at output tau
            const int64_t sq = (int64_t)floor(256.0 * (hT + hA) + 0.5);
            D = (sq + 255) >> 8;
            w = (c & 255) + 256 * (256 * D - sq) + PV_CHOIR_MIRROR_BIT;
            if (D > INT32_MAX) past = true;
        } else {
            const int64_t dq = (int64_t)floor(256.0 * (hT - hA) + 0.5);
            D = dq >> 8;
            w = (c & 255) + 256 * (dq & 255);
        }
        if (s != PV_TSM_Q) w = w + (s << PV_CHOIR_STEP_SHIFT);
        if (m < capacity && !past) {
            grains[4 * m + 0] = (int32_t)(c >> 8);
            grains[4 * m + 1] = (int32_t)w;
            grains[4 * m + 2] = (int32_t)D;
            grains[4 * m + 3] = (int32_t)L;
        }
        m++;
    };
    while (V < len && !past) {
        while (fabs(An - V) < fabs(A - V)) {                            // the analysis mark nearest V, ties to the lower: a monotone walk
            A = An;
            An = tr.snap(A + tr.period(A), &A);
        }
        // pv_tsm_plan's unvoiced rule: the read position goes onto the analysis mark and the synthesis mark moves with it
        if (held && !tr.voiced(V) && !tr.voiced(A) && A < len) {
            const double Tn = A + rint((T + (A - V)) - A);
            if (A >= Vprev + 1.0 && Tn >= Tprev + 1.0 && Tn - Tprev <= far) { T = Tn; V = A; }
        }
        if (held) emit(T - hT);
        // a reuse (the grain before it sits on this very mark, and the mark is unvoiced or there are no records) takes the other direction
        const bool reuse = mirror != 0 && held && hA == A && !tr.voiced(A);
        hmir = reuse && !hmir;
        hgap = held ? T - hT : 0.0;
        hT = T; hA = A; hV = V; held = true;
        Tprev = T; Vprev = V;
        const double s = tr.step(V);
        T = T + s;
        V = V + tr.rate(V) * s;
    }
    if (held) emit(T - hT);
    if (past) return -PV_ERR_ARGUMENT;
    if (output_len) *output_len = held ? (int64_t)floor(hT + (len - hV) / tr.rate(hV) + 0.5) : 0;
    return m;
}

}  // extern "C"
