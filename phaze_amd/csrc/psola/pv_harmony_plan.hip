// pv_harmony_plan.hip -- pv_harmony_ratios of include/phaze_amd.h: from the tracker's records to one pitch ratio per (voice, record), every voice a
// number of scale degrees away from the corrected lead.  Pure host code: no handle, no device.  The rule is DESIGN.md "Harmony voices";
// tests/harmony_model.py restates it in Python and tests/test_harmony_abi.py compares the two exactly, so the arithmetic below is written one operation
// at a time: no contraction, and pow stays pow (as pv_psola_plan.hip, whose one-pole is restated here operation for operation).
#include <math.h>
#include <stdint.h>

#include "../../../include/phaze_amd.h"
#include "pv_harmony.h"

#pragma clang fp contract(off)

namespace {

double (*volatile pv_pow)(double, double) = pow;                       // an optimiser that knows pow(2, r) would call exp2: another function, other bits

constexpr int kMaxDegree = 24;

bool allowed(int32_t mask, int64_t note) { return mask >> (int)(((note % 12) + 12) % 12) & 1; }

}  // namespace

extern "C" {

int64_t pv_harmony_ratios(const pv_tune_params *p, const int32_t *records, int64_t nrec, const int32_t *degrees, int32_t nvoices, double *ratios, int64_t capacity)
{
    if (!p || p->struct_size != (int32_t)sizeof(pv_tune_params) || nrec < 0 || (nrec > 0 && !records) || capacity < 0 || (capacity > 0 && !ratios))
        return -PV_ERR_ARGUMENT;
    const double a4 = p->a4 == 0.0 ? 440.0 : p->a4;
    if (!(p->sample_rate > 0.0) || !(a4 > 0.0) || !isfinite(p->sample_rate) || !isfinite(a4) || p->scale_mask < 1 || p->scale_mask > 0xFFF
        || !(p->strength >= 0.0 && p->strength <= 1.0) || !(p->retune > 0.0 && p->retune <= 1.0) || p->reserved != 0)
        return -PV_ERR_ARGUMENT;
    if (nvoices < 1 || nvoices > PV_HARMONY_MAX_VOICES || !degrees) return -PV_ERR_ARGUMENT;
    for (int32_t v = 0; v < nvoices; v++)
        if (degrees[v] < -kMaxDegree || degrees[v] > kMaxDegree) return -PV_ERR_ARGUMENT;
    double r = 0.0;
    for (int64_t j = 0; j < nrec; j++) {
        double t = 0.0;
        int64_t note = 0;                                                // ns, the allowed note the lead is corrected onto
        bool voiced = false;
        const double period = pv_f0_period(records + 4 * j);
        if (period > 0.0) {
            const double n = 69.0 + 12.0 * log2(p->sample_rate / period / a4);
            int64_t lo = (int64_t)floor(n), hi = lo + 1;                 // the allowed notes on either side of n; C is pitch class 0 of note 0
            while (!allowed(p->scale_mask, lo)) lo--;
            while (!allowed(p->scale_mask, hi)) hi++;
            note = n - (double)lo <= (double)hi - n ? lo : hi;
            const double ns = (double)note;
            t = p->strength * (ns - n) / 12.0;
            voiced = true;
        }
        r += p->retune * (t - r);
        if (j >= capacity) continue;
        for (int32_t v = 0; v < nvoices; v++) {
            int64_t m = note;
            if (voiced)
                for (int32_t left = degrees[v] < 0 ? -degrees[v] : degrees[v]; left > 0;) {          // |k| allowed notes up or down from ns
                    m += degrees[v] < 0 ? -1 : 1;
                    if (allowed(p->scale_mask, m)) left--;
                }
            const double interval = (double)(m - note) / 12.0;           // i / 12: 0 for degree 0 and for unvoiced or empty records
            double ratio = pv_pow(2.0, r + interval);
            if (ratio < 0.5) ratio = 0.5;
            if (ratio > 2.0) ratio = 2.0;
            ratios[v * capacity + j] = ratio;
        }
    }
    return nrec;
}

}  // extern "C"
