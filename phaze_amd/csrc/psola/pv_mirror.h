// pv_mirror.h -- host <-> kernel contract of mirrored grains on the overlap-add path (pv_mirror_*, include/phaze_amd.h).
//
// A grain is four int32 {t, w, D, L} with w = tf + 256 phi + 65536 m, tf and phi in 0 .. 255, m in {0, 1}.  With m = 0 it is pv_tsm.h's far grain
// word for word (|D| < 2^30): output n of the grain reads the input at the real position n - D - phi / 256.  With m = 1 the grain is MIRRORED: output n
// reads the input at D - n - phi / 256, so it plays its stretch of the input backwards; D > -2^30, and any larger int32 is allowed (D is a sum of two
// positions below 2^30).  0 <= w < 131072, 2 <= L <= max_period <= 4096, 0 <= t < 2^30, centres non-decreasing on 256 t + tf.  With Q = 256:
//   window   as pv_tsm.h: ua = |256 (n - t) - tf|, weight 0 when ua >= 256 L, else q = (4 ua) div L, rem = (4 ua) mod L,
//            f = f32(rem) * (1.0f / f32(L)), h = fmaf(f, Hn[q + 1] - Hn[q], Hn[q]).
//   sample   m = 0: pv_tsm.h's.  m = 1: that rule with n - D replaced by D - n and nothing else.  phi == 0: xt = x[D - n].  Else theta = 256 - phi,
//            b = D - n - 1, the taps i = 0 .. 63 read x[b - 31 + i] with weight w_i = P[|256 (i - 31) - theta|]; a = s = 0, for i ascending
//            a = fmaf(w_i, x_i, a) and s = s + w_i, then xt = a / s.  x is 0 outside [0, nin).  (The real position is b + theta / 256, so tap i lies
//            (i - 31) - theta / 256 samples from it: the weights are the forward grain's.)
//   output   as pv_tsm.h: num and den in grain order, a grain whose h is exactly 0 touches neither sum, an uncovered output is exactly 0.
// SUMMATION ORDER: a function of (g, i) alone, so any partition of the output range gives the same bits.  NON-FINITE INPUT: as pv_psola.h.
//
// TILES.  One workgroup per (tile of PV_TSM_TILE outputs, channel), one int4 {g_first, g_end, src0, src_count} per tile [j0, j1).  The grain range
// [g_first, g_end) is pv_tsm's walk: it depends on t and L only.  A forward grain that reaches the tile has pv_tsm.h's source range,
//   lo = max(j0, t - L) - D - 33,  hi = min(j1, t + L) - D + 32;
// a mirrored one has
//   lo = D - min(j1, t + L) - 33,  hi = D - max(j0, t - L) + 32.
// src0 = min lo, src_count = max hi - min lo over both kinds; {a, b, 0, 0} for a tile no grain reaches.  Why every tap of a covered output lies in
// [lo + 1, hi - 1] for a mirrored grain: a covered output n of the tile has ua < 256 L, so t - L < n <= t + L (n = t + L only with tf > 0), and
// j0 <= n < j1: n1 := max(j0, t - L + 1) <= n <= min(j1 - 1, t + L) =: n2.  Its taps are the positions D - n - 32 .. D - n + 31 (one position, D - n,
// for phi == 0).  The lowest is D - n2 - 32 = D - min(j1, t + L + 1) - 31 >= D - min(j1, t + L) - 32 = lo + 1; the highest is
// D - n1 + 31 = D - max(j0 - 1, t - L) + 30 <= D - max(j0, t - L) + 31 = hi - 1.  (The forward grain's derivation, pv_tsm.h, with the two ends swapped.)
// The host refuses a call with a tile whose src_count exceeds pv_tsm_span(max_period, max_rate); the formula and the 160 KiB rule are pv_tsm's.
// LDS: pv_tsm.h's layout (the padded span, then P, then Hn).  Every LDS index is clamped to the staged count, in both directions.
//
// Validation and the tile walk are inline host functions here, so that the handle (pv_mirror_capi.hip) and a host-only build share one text.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "pv_tsm.h"

#define PV_MIRROR_BIT (PV_TSM_Q * PV_TSM_Q)            // bit 16 of w

// Asynchronous on `stream`.  The parameters are pv_tsm's: the direction travels in the grain records.
hipError_t pv_launch_mirror(const PvTsmParams &p, hipStream_t stream);

// why a grain is refused
enum { PV_MIRROR_BAD_CENTRE = 1, PV_MIRROR_BAD_LENGTH = 2, PV_MIRROR_BAD_SHIFT = 3, PV_MIRROR_BAD_ORDER = 4 };

// The index of the first grain that breaks a rule and *why, or -1.
static inline int64_t pv_mirror_check_grains(const int32_t *grains, int64_t ngrains, int max_period, int *why)
{
    long long prev = 0;
    for (int64_t g = 0; g < ngrains; g++) {
        const int32_t t = grains[4 * g], w = grains[4 * g + 1], D = grains[4 * g + 2], L = grains[4 * g + 3];
        int bad = 0;
        const long long c = (long long)t * PV_TSM_Q + (w & (PV_TSM_Q - 1));
        if (t < 0 || t >= PV_TSM_MAX_POSITION || w < 0 || w >= 2 * PV_MIRROR_BIT) bad = PV_MIRROR_BAD_CENTRE;
        else if (L < 2 || L > max_period) bad = PV_MIRROR_BAD_LENGTH;
        else if (D <= -PV_TSM_MAX_POSITION || (!(w & PV_MIRROR_BIT) && D >= PV_TSM_MAX_POSITION)) bad = PV_MIRROR_BAD_SHIFT;
        else if (c < prev) bad = PV_MIRROR_BAD_ORDER;
        if (bad) {
            if (why) *why = bad;
            return g;
        }
        prev = c;
    }
    return -1;
}

// The tiles of outputs [out_first, out_first + nout) of a validated table: tiles[4 k ..] = {g_first, g_end, src0, src_count} of tile k in int64, as
// tests/mirror_model.py's tiles().  Returns the number of tiles.
static inline int64_t pv_mirror_tiles(const int32_t *grains, int64_t ngrains, int max_period, int64_t out_first, int64_t nout, int64_t *tiles)
{
    const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE, mp = max_period;
    long long lo = 0, hi = 0;
    for (long long k = 0; k < ntiles; k++) {
        const long long j0 = out_first + k * PV_TSM_TILE, j1 = j0 + (nout - k * PV_TSM_TILE < PV_TSM_TILE ? nout - k * PV_TSM_TILE : PV_TSM_TILE);
        // centres are in order and no half length is above max_period: a grain that reaches [j0, j1) has its centre t within [j0 - mp - 1, j1 + mp)
        while (lo < ngrains && grains[4 * lo] < j0 - mp - 1) lo++;
        if (hi < lo) hi = lo;
        while (hi < ngrains && grains[4 * hi] < j1 + mp) hi++;
        long long a = lo, b = hi;                                       // trimmed to the first and the last grain that reach the tile
        while (a < b && (long long)grains[4 * a] + 1 + grains[4 * a + 3] <= j0) a++;
        while (b > a && (long long)grains[4 * (b - 1)] - grains[4 * (b - 1) + 3] >= j1) b--;
        long long s0 = 0, s1 = 0;
        bool any = false;
        for (long long g = a; g < b; g++) {
            const long long c = grains[4 * g], D = grains[4 * g + 2], L = grains[4 * g + 3];
            if (c + L < j0 || c - L >= j1) continue;                    // cannot cover an output of the tile
            const long long first = j0 > c - L ? j0 : c - L, last = j1 < c + L ? j1 : c + L;
            const bool m = (grains[4 * g + 1] & PV_MIRROR_BIT) != 0;
            const long long from = (m ? D - last : first - D) - PV_TSM_TAPS / 2 - 1, to = (m ? D - first : last - D) + PV_TSM_TAPS / 2;
            if (!any || from < s0) s0 = from;
            if (!any || to > s1) s1 = to;
            any = true;
        }
        tiles[4 * k] = a;
        tiles[4 * k + 1] = b;
        tiles[4 * k + 2] = s0;
        tiles[4 * k + 3] = s1 - s0;
    }
    return ntiles;
}

// src0 as the kernel gets it.  A mirrored grain with D near -2^30 on outputs near 2^30 reads from up to 32 samples below -2^31; such a span lies wholly
// below the input and holds zeros at every index, so holding its origin at INT32_MIN changes nothing that is read.
static inline int32_t pv_mirror_src0(int64_t s0) { return s0 < INT32_MIN ? INT32_MIN : (int32_t)s0; }
