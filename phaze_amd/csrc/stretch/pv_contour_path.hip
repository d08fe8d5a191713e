// pv_contour_path.hip -- pv_contour_path of include/phaze_amd.h: the cheapest path through a candidate table.  Pure host code in integers: no handle, no
// device, no HIP call (it also compiles as plain C++).  The rules are DESIGN.md "Pitch contour"; tests/contour_model.py restates them in Python and
// tests/test_contour_abi.py compares the two exactly.  The bound on the int64 costs is stated in pv_contour.h.
#include <stdint.h>
#include <stdlib.h>

#include "../../../include/phaze_amd.h"

namespace {

constexpr int KMAX = 8;
constexpr int64_t NONE = INT64_MAX;                                       // the cost of what is not a state
constexpr int64_t C_CAP = 1 << 14;

}  // namespace

extern "C" int pv_contour_path(const pv_contour_params *p, const int32_t *candidates, int64_t nrec, int32_t *records, int32_t *states)
{
    if (!p || p->struct_size != (int32_t)sizeof(pv_contour_params) || p->reserved != 0) return PV_ERR_ARGUMENT;
    if (p->candidates < 1 || p->candidates > KMAX || p->max_lag < 3 || p->max_lag > 4096 || p->bias < 0 || p->bias > 16384 || p->unvoiced_cost < 1
        || p->unvoiced_cost > 16384 || p->voicing_cost < 0 || p->voicing_cost > (1 << 20) || p->jump_cost < 0 || p->jump_cost > (1 << 20))
        return PV_ERR_ARGUMENT;
    if (nrec < 0 || nrec > 0x7fffffff) return PV_ERR_ARGUMENT;
    if (nrec == 0) return PV_OK;
    if (!candidates || !records) return PV_ERR_ARGUMENT;
    const int K = p->candidates;
    const int64_t bias = p->bias, ML = p->max_lag, jump2 = 2 * (int64_t)p->jump_cost, vc = p->voicing_cost;
    for (int64_t i = 0; i < nrec * K; i++) {                              // the whole table before anything is written
        const int32_t *c = candidates + 4 * i;
        if (c[0] < 0 || c[0] > 65535 || c[1] < 0 || c[2] < 0 || c[3] < 0) return PV_ERR_ARGUMENT;
    }
    uint8_t *back = (uint8_t *)malloc((size_t)nrec * (size_t)(K + 1));
    if (!back) return PV_ERR_DEVICE;

    int64_t D[KMAX + 1], E[KMAX + 1];
    for (int64_t m = 0; m < nrec; m++) {
        const int32_t *cur = candidates + 4 * K * m, *prev = m > 0 ? cur - 4 * K : cur;
        uint8_t *bk = back + m * (K + 1);
        for (int s = 0; s <= K; s++) {
            int64_t o;                                                    // the observation cost, NONE for an empty slot
            if (s == K) o = cur[0] > 0 ? p->unvoiced_cost : 0;
            else if (cur[4 * s] > 0) o = (cur[4 * s + 2] < C_CAP ? cur[4 * s + 2] : C_CAP) + bias * cur[4 * s] / ML;
            else o = NONE;
            bk[s] = 0;
            if (m == 0 || o == NONE) { E[s] = o; continue; }
            int64_t best = NONE;
            for (int a = 0; a <= K; a++) {                                // ascending, strict <: a tie stays with the lowest a
                if (D[a] == NONE) continue;
                int64_t t;
                if (a == K || s == K) t = a == s ? 0 : vc;
                else {
                    const int64_t ta = prev[4 * a], tb = cur[4 * s];
                    t = jump2 * (tb > ta ? tb - ta : ta - tb) / (ta + tb);
                }
                if (D[a] + t < best) { best = D[a] + t; bk[s] = (uint8_t)a; }
            }
            E[s] = o + best;                                              // the unvoiced state always exists: best is a cost
        }
        for (int s = 0; s <= K; s++) D[s] = E[s];
    }
    int s = K;
    for (int a = K - 1; a >= 0; a--)
        if (D[a] <= D[s]) s = a;                                          // the first argmin (D[K] is never NONE)
    for (int64_t m = nrec - 1; m >= 0; m--) {
        const int32_t *cur = candidates + 4 * K * m;
        int32_t *r = records + 4 * m;
        if (s < K) { r[0] = cur[4 * s]; r[1] = cur[4 * s + 1]; r[2] = cur[4 * s + 2]; r[3] = cur[4 * s + 3]; }
        else if (cur[0] > 0) { r[0] = -cur[0]; r[1] = cur[1]; r[2] = cur[2]; r[3] = cur[3]; }
        else r[0] = r[1] = r[2] = r[3] = 0;
        if (states) states[m] = s;
        s = back[m * (K + 1) + s];
    }
    free(back);
    return PV_OK;
}
