// pv_psola_plan.hip -- pv_psola_ratios and pv_psola_plan of include/phaze_amd.h: from the tracker's records to one pitch ratio per record, and from
// records and ratios to the grain table of pv_psola_process.  Pure host code: no handle, no device.  The rules are DESIGN.md "Pitch-synchronous
// correction"; tests/psola_model.py restates them in Python and tests/test_psola_abi.py compares the two exactly, so the arithmetic below is written
// one operation at a time: no contraction, and pow stays pow (as pv_tune_plan.hip).
#include <math.h>
#include <stdint.h>

#include "../../../include/phaze_amd.h"
#include "pv_psola.h"

#pragma clang fp contract(off)

namespace {

double (*volatile pv_pow)(double, double) = pow;                       // an optimiser that knows pow(2, r) would call exp2: another function, other bits

int64_t floor_div(int64_t a, int64_t b)                                 // b > 0
{
    const int64_t q = a / b;
    return a % b < 0 ? q - 1 : q;
}

struct Track {
    const pv_psola_params *p;
    const int32_t *records;
    const double *ratios;
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
    // the largest distance between two synthesis marks: two grains of the longest half length still cover everything between their centres
    double cap() const { return p->max_period > 2 ? (double)(2 * p->max_period - 4) : 1.0; }
    // the distance to the next synthesis mark: period / ratio, at most cap()
    double step(double tau) const
    {
        const double s = period(tau) / ratio(tau);
        return s < cap() ? s : cap();
    }
};

}  // namespace

extern "C" {

int64_t pv_psola_ratios(const pv_tune_params *p, const int32_t *records, int64_t nrec, double *ratios, int64_t capacity)
{
    if (!p || p->struct_size != (int32_t)sizeof(pv_tune_params) || nrec < 0 || (nrec > 0 && !records) || capacity < 0 || (capacity > 0 && !ratios))
        return -PV_ERR_ARGUMENT;
    const double a4 = p->a4 == 0.0 ? 440.0 : p->a4;
    if (!(p->sample_rate > 0.0) || !(a4 > 0.0) || !isfinite(p->sample_rate) || !isfinite(a4) || p->scale_mask < 1 || p->scale_mask > 0xFFF
        || !(p->strength >= 0.0 && p->strength <= 1.0) || !(p->retune > 0.0 && p->retune <= 1.0) || p->reserved != 0)
        return -PV_ERR_ARGUMENT;
    double r = 0.0;
    for (int64_t j = 0; j < nrec; j++) {
        double t = 0.0;
        const double period = pv_f0_period(records + 4 * j);
        if (period > 0.0) {
            const double n = 69.0 + 12.0 * log2(p->sample_rate / period / a4);
            int64_t lo = (int64_t)floor(n), hi = lo + 1;                 // the allowed notes on either side of n; C is pitch class 0 of note 0
            while (!(p->scale_mask >> (int)(((lo % 12) + 12) % 12) & 1)) lo--;
            while (!(p->scale_mask >> (int)(((hi % 12) + 12) % 12) & 1)) hi++;
            const double ns = n - (double)lo <= (double)hi - n ? (double)lo : (double)hi;
            t = p->strength * (ns - n) / 12.0;
        }
        r += p->retune * (t - r);
        double ratio = pv_pow(2.0, r);
        if (ratio < 0.5) ratio = 0.5;
        if (ratio > 2.0) ratio = 2.0;
        if (j < capacity) ratios[j] = ratio;
    }
    return nrec;
}

int64_t pv_psola_plan(const pv_psola_params *p, const int32_t *records, int64_t nrec, const double *ratios, int32_t *grains, int64_t capacity)
{
    if (!p || p->struct_size != (int32_t)sizeof(pv_psola_params) || nrec < 0 || (nrec > 0 && !records) || capacity < 0 || (capacity > 0 && !grains))
        return -PV_ERR_ARGUMENT;
    if (p->f0_hop < 1 || p->min_period < 2 || p->max_period < p->min_period || p->max_period > PV_PSOLA_MAX_PERIOD || p->reserved != 0
        || !(p->unvoiced_period >= (double)p->min_period && p->unvoiced_period <= (double)p->max_period) || p->input_len < 0
        || p->input_len >= PV_PSOLA_MAX_POSITION)
        return -PV_ERR_ARGUMENT;
    if (ratios)
        for (int64_t j = 0; j < nrec; j++)
            if (!(ratios[j] >= 0.5 && ratios[j] <= 2.0)) return -PV_ERR_ARGUMENT;
    const Track tr{p, records, ratios, nrec};
    const double len = (double)p->input_len, far = tr.cap();
    double A = 0.0, An = A + tr.period(A);                              // the analysis mark in hand and the one after it
    double T = 0.0, Tprev = 0.0;
    int64_t m = 0;
    // one grain is held back until the mark after it is final: its half length covers half the way to either neighbour
    bool held = false;
    double hT = 0.0, hA = 0.0, hgap = 0.0;
    const auto emit = [&](double gap_after) {
        double L = floor(tr.period(hA) + 0.5);
        const double g = hgap > gap_after ? hgap : gap_after, need = floor(g / 2.0) + 2.0;
        if (L < need) L = need;
        if (L < 2.0) L = 2.0;
        if (L > (double)p->max_period) L = (double)p->max_period;
        if (m < capacity) {
            const int64_t c = (int64_t)floor(256.0 * hT + 0.5);
            grains[4 * m + 0] = (int32_t)(c >> 8);
            grains[4 * m + 1] = (int32_t)(c & 255);
            grains[4 * m + 2] = (int32_t)floor(256.0 * (hT - hA) + 0.5);
            grains[4 * m + 3] = (int32_t)L;
        }
        m++;
    };
    while (T < len) {
        while (fabs(An - T) < fabs(A - T)) {                            // the analysis mark nearest T, ties to the lower: a monotone walk
            A = An;
            An = A + tr.period(A);
        }
        // inside an unvoiced stretch the synthesis mark snaps onto the analysis mark, so that the material passes unshifted
        // (never closer than one sample to the mark before it, never further than cap() from it)
        if (held && !tr.voiced(T) && !tr.voiced(A) && A < len && A >= Tprev + 1.0 && A - Tprev <= far) T = A;
        if (held) emit(T - hT);
        hgap = held ? T - hT : 0.0;
        hT = T; hA = A; held = true;
        Tprev = T;
        T = T + tr.step(T);
    }
    if (held) emit(T - hT);
    return m;
}

}  // extern "C"
