// pv_tune_plan.hip -- pv_f0_period and pv_tune_plan of include/phaze_amd.h: from the tracker's records to periods, and from periods to the hop row of
// pv_glide_process that moves every frame onto the nearest note of a scale.  Pure host code: no handle, no device.  The rules are DESIGN.md "Pitch
// tracking"; tests/f0_model.py restates them in Python and tests/test_f0_abi.py compares the two exactly, so the arithmetic below is written one
// operation at a time: no contraction, and pow stays pow.
#include <math.h>
#include <stdint.h>

#include "../../../include/phaze_amd.h"

#pragma clang fp contract(off)

namespace {

double (*volatile pv_pow)(double, double) = pow;                       // an optimiser that knows pow(2, r) would call exp2: another function, other bits

int64_t floor_div(int64_t a, int64_t b)                                 // b > 0
{
    const int64_t q = a / b;
    return a % b < 0 ? q - 1 : q;
}

}  // namespace

extern "C" {

double pv_f0_period(const int32_t rec[4])
{
    if (!rec || rec[0] <= 0) return 0.0;
    const int64_t num = (int64_t)rec[1] - (int64_t)rec[3];
    const int64_t den = (int64_t)rec[1] - 2 * (int64_t)rec[2] + (int64_t)rec[3];
    if (den <= 0) return (double)rec[0];
    return (double)rec[0] + 0.5 * (double)num / (double)den;
}

int64_t pv_tune_plan(const pv_tune_params *p, const int32_t *records, int64_t nrec, int32_t *hops, double *curve, int64_t capacity)
{
    if (!p || p->struct_size != (int32_t)sizeof(pv_tune_params) || nrec < 0 || (nrec > 0 && !records) || capacity < 0 || (capacity > 0 && !hops))
        return -PV_ERR_ARGUMENT;
    const double a4 = p->a4 == 0.0 ? 440.0 : p->a4;
    if (p->f0_hop < 1 || !(p->sample_rate > 0.0) || !(a4 > 0.0) || !isfinite(p->sample_rate) || !isfinite(a4) || p->scale_mask < 1 || p->scale_mask > 0xFFF
        || !(p->strength >= 0.0 && p->strength <= 1.0) || !(p->retune > 0.0 && p->retune <= 1.0) || p->synthesis_hop < 1 || p->min_hop < 1
        || p->max_hop < p->min_hop || p->input_len < 0 || p->reserved != 0)
        return -PV_ERR_ARGUMENT;
    const int64_t fh = p->f0_hop;
    const double hs = (double)p->synthesis_hop;
    int64_t S = 0, m = 0;
    double r = 0.0, e = 0.0;
    for (;;) {
        double t = 0.0;
        if (nrec > 0) {
            int64_t j = floor_div(S + p->shift - p->f0_center + fh / 2, fh);
            if (j < 0) j = 0;
            if (j > nrec - 1) j = nrec - 1;
            const double period = pv_f0_period(records + 4 * j);
            if (period > 0.0) {
                const double n = 69.0 + 12.0 * log2(p->sample_rate / period / a4);
                int64_t lo = (int64_t)floor(n), hi = lo + 1;             // the allowed notes on either side of n; C is pitch class 0 of note 0
                while (!(p->scale_mask >> (int)(((lo % 12) + 12) % 12) & 1)) lo--;
                while (!(p->scale_mask >> (int)(((hi % 12) + 12) % 12) & 1)) hi++;
                const double ns = n - (double)lo <= (double)hi - n ? (double)lo : (double)hi;
                t = p->strength * (ns - n) / 12.0;
            }
        }
        r += p->retune * (t - r);
        const double x = e + hs / pv_pow(2.0, r);
        double h = floor(x + 0.5);
        if (h < (double)p->min_hop) h = (double)p->min_hop;
        if (h > (double)p->max_hop) h = (double)p->max_hop;
        const int64_t hop = (int64_t)h;
        e = x - (double)hop;
        if (S + hop > p->input_len) break;
        if (m < capacity) {
            hops[m] = (int32_t)hop;
            if (curve) curve[m] = r;
        }
        S += hop;
        m++;
    }
    return m;
}

}  // extern "C"
