// pv_formant.h -- host <-> kernel contract of warped grains on the overlap-add path (pv_formant_*, include/phaze_amd.h): formant shifting.
//
// A grain is four int32 {t, w, D, L} with w = tf + 256 phi + 131072 z, tf and phi in 0 .. 255.  Bit 16, pv_mirror.h's direction bit, must be 0 here.
// z, bits 17 .. 26 of w, is the STEP s of the grain in 1/256: z = 0 means s = 256, else 128 <= z <= 512 and s = z; z = 256 is legal and is treated exactly
// as z = 0.  A grain is refused with PV_FORMANT_BAD_STEP when w < 0 or w >= 2^27, when z lies in 1 .. 127 or above 512, or when bit 16 is set.  Everything
// else in the grain rules is pv_tsm.h's: 0 <= t < 2^30, 2 <= L <= max_period <= 4096, |D| < 2^30, centres non-decreasing on 256 t + tf.
// A grain with s = 256 is pv_tsm.h's far grain word for word (phi == 0 reads the sample itself), and a table with no warped grain gives pv_tsm_process's
// bits.  A grain with s != 256 is WARPED: output n of the grain reads the input at the real position
//     (t + tf / 256 - D - phi / 256) + (s / 256) (n - t - tf / 256),
// the position the unwarped grain reads at its centre, and from there s / 256 input samples per output sample: the grain is its stretch of the input
// time-compressed (s > 256) or time-expanded (s < 256), which scales its spectrum, and so the envelope, by s / 256; the grain spacing still sets the pitch.
// In exact integers:
//   position u = 256 (n - t) - tf (|u| < 2^20 for a covered output, so |s u| < 2^29); v = 256 (tf - phi) + s u in int32; m = (t - D) + floor(v / 65536),
//            formed in wrapping unsigned arithmetic as pv_mirror_kernel forms its index; r = v mod 65536 in 0 .. 65535.  The position is m + r / 65536.
//   weights  den = max(256, s); W = 32 for s <= 256 and 64 otherwise.  Tap i = 0 .. 2 W - 1 reads x[m - W + 1 + i] and lies d / 65536 samples from the
//            position, d = |(i - W + 1) 65536 - r|.  q = d div den, rem = d mod den; w_i = 0 when q >= 32 * 256, else f = f32(rem) * (1.0f / f32(den)) and
//            w_i = fmaf(f, P[q + 1] - P[q], P[q]): pv_vari.h's weight rule with d in the place of a Q.  At s > 256 the prototype is widened by s / 256, which
//            lowers the cutoff by 256 / s: a compressed grain does not alias.  (At s = 256 the rule gives pv_tsm's weights: r is a multiple of 256, rem = 0
//            and q = |256 (i - 31) - theta|.  That is why the two kinds may share a table.)
//   sample   a = sum = 0; for i ascending a = fmaf(w_i, x_i, a) and sum = sum + w_i; xt = a / sum.  A tap whose weight is exactly 0 touches neither sum,
//            WHATEVER its sample holds (pv_vari.h's non-finite rule), so a launch may skip the taps that are 0 for every output: only
//            -K <= i - W + 1 <= K + 1 with K = ceil(den / 8) - 1 can be non-zero (d >= |i - W + 1| 65536 - 65535, and w_i = 0 from d = 8192 den on).
//            x is 0 outside [0, nin).
//   window, output fold (num, den, grains in order), the zero for uncovered outputs and the SUMMATION ORDER clause: pv_tsm.h's.
//
// TILES.  One workgroup per (tile of PV_TSM_TILE outputs, channel), one int4 {g_first, g_end, src0, src_count} per tile [j0, j1).  The grain range is
// pv_tsm's walk (t and L only).  An unwarped grain that reaches the tile has pv_tsm.h's source range.  For a warped one let
//     M(n) = (t - D) + floor((256 (tf - phi) + s (256 (n - t) - tf)) / 65536),
// the m of output n; then
//     lo = M(max(j0, t - L)) - W - 1,  hi = M(min(j1, t + L)) + W + 1.
// Why every tap of a covered output lies in [lo + 1, hi - 1]: a covered output n of the tile has max(j0, t - L) <= n <= min(j1, t + L) (pv_mirror.h), and M
// does not decrease with n since s > 0, so M(max(j0, t - L)) <= M(n) <= M(min(j1, t + L)).  The taps of n are M(n) - W + 1 .. M(n) + W: the lowest is at least
// lo + 2 and the highest at most hi - 1.  src0 = min lo and src_count = max hi - min lo over the tile's grains of both kinds.
//
// SPAN.  pv_formant_span(max_period, max_rate) = max_rate (PV_TSM_TILE + 2 max_period) + 6 max_period + 192 staged samples per tile at most; the host
// refuses a call with a tile beyond it, before any device work.  It is pv_tsm_span's budget with two terms wider.  The grains that reach a tile have their
// centres in a range of PV_TSM_TILE + 2 max_period outputs, the read position runs at most max_rate times as fast as the synthesis position, and a mark is
// within a period of the read position it serves on either side (2 max_period with the snap): so far pv_tsm's.  A grain of pv_tsm_plan reads L <= max_period
// to either side of its mark; a grain of pv_formant_plan reads (s / 256) L, and its L is min(max_period, max(round(period 256 / s), floor(gap / 2) + 2, 2))
// with gap <= 2 max_period - 4, so (s / 256) L <= max(period + 1, (s / 256) max_period) <= 2 max_period for s <= 512: 4 max_period for the two sides where
// pv_tsm has 2.  The taps and the two guard samples of lo and hi are 2 (64 + 1) + 1 where pv_tsm has 65; 192 covers them and the roundings of M.  So a table
// of pv_formant_plan with rates within [1 / max_rate, max_rate] and steps within [1/2, 2] keeps to it (tests/test_formant_model.py sweeps the corners).
// The span, P and Hn share the 160 KiB of LDS of a compute unit, so fewer (max_period, max_rate) pairs fit than pv_tsm's: max_period up to 3753 at
// max_rate 1, 2900 at 2, 2331 at 3 and 1925 at 4; pv_formant_create returns PV_ERR_UNSUPPORTED beyond.
// LDS: pv_tsm.h's layout (the padded span, then P, then Hn).  Every LDS index is clamped to the staged count.
//
// Validation, the tile walk and src0 are inline host functions here, so that the handle (pv_formant_capi.hip) and a host-only build share one text.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "pv_tsm.h"

#define PV_FORMANT_MIRROR_BIT (PV_TSM_Q * PV_TSM_Q)    // bit 16 of w: must be 0
#define PV_FORMANT_STEP_SHIFT 17                       // z = (w >> 17) & 1023
#define PV_FORMANT_W_END (1 << 27)
#define PV_FORMANT_MIN_STEP 128
#define PV_FORMANT_MAX_STEP 512
#define PV_FORMANT_TAPS 128                            // taps of a warped grain at most (s > 256); 64 for s < 256

// Asynchronous on `stream`.  The parameters are pv_tsm's: the step travels in the grain records.
hipError_t pv_launch_formant(const PvTsmParams &p, hipStream_t stream);

// why a grain is refused
enum { PV_FORMANT_BAD_CENTRE = 1, PV_FORMANT_BAD_LENGTH = 2, PV_FORMANT_BAD_SHIFT = 3, PV_FORMANT_BAD_ORDER = 4, PV_FORMANT_BAD_STEP = 5 };

// the step of a valid w: 256 for z = 0
static inline __host__ __device__ int pv_formant_step(int32_t w)
{
    const int z = (w >> PV_FORMANT_STEP_SHIFT) & 1023;
    return z ? z : PV_TSM_Q;
}

static inline __host__ __device__ int pv_formant_span(int max_period, int max_rate) { return max_rate * (PV_TSM_TILE + 2 * max_period) + 6 * max_period + 192; }

// The index of the first grain that breaks a rule and *why, or -1.
static inline int64_t pv_formant_check_grains(const int32_t *grains, int64_t ngrains, int max_period, int *why)
{
    long long prev = 0;
    for (int64_t g = 0; g < ngrains; g++) {
        const int32_t t = grains[4 * g], w = grains[4 * g + 1], D = grains[4 * g + 2], L = grains[4 * g + 3];
        int bad = 0;
        const long long c = (long long)t * PV_TSM_Q + (w & (PV_TSM_Q - 1));
        const int z = w >= 0 ? (w >> PV_FORMANT_STEP_SHIFT) : 0;
        if (t < 0 || t >= PV_TSM_MAX_POSITION) bad = PV_FORMANT_BAD_CENTRE;
        else if (w < 0 || w >= PV_FORMANT_W_END || (w & PV_FORMANT_MIRROR_BIT) || (z != 0 && (z < PV_FORMANT_MIN_STEP || z > PV_FORMANT_MAX_STEP))) bad = PV_FORMANT_BAD_STEP;
        else if (L < 2 || L > max_period) bad = PV_FORMANT_BAD_LENGTH;
        else if (D <= -PV_TSM_MAX_POSITION || D >= PV_TSM_MAX_POSITION) bad = PV_FORMANT_BAD_SHIFT;
        else if (c < prev) bad = PV_FORMANT_BAD_ORDER;
        if (bad) {
            if (why) *why = bad;
            return g;
        }
        prev = c;
    }
    return -1;
}

// M(n) of a warped grain, in int64 (the contract above)
static inline long long pv_formant_m(long long t, int tf, int phi, long long D, int s, long long n)
{
    const long long v = 256LL * (tf - phi) + (long long)s * (256LL * (n - t) - tf);
    return (t - D) + (v >> 16);                                         // an arithmetic shift: floor
}

// The tiles of outputs [out_first, out_first + nout) of a validated table: tiles[4 k ..] = {g_first, g_end, src0, src_count} of tile k in int64, as
// tests/formant_model.py's tiles().  Returns the number of tiles.
static inline int64_t pv_formant_tiles(const int32_t *grains, int64_t ngrains, int max_period, int64_t out_first, int64_t nout, int64_t *tiles)
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
            const int32_t w = grains[4 * g + 1];
            const int s = pv_formant_step(w);
            long long from, to;
            if (s == PV_TSM_Q) {
                from = first - D - PV_TSM_TAPS / 2 - 1;
                to = last - D + PV_TSM_TAPS / 2;
            } else {
                const int W = s < PV_TSM_Q ? PV_TSM_TAPS / 2 : PV_FORMANT_TAPS / 2, tf = w & (PV_TSM_Q - 1), phi = (w >> 8) & (PV_TSM_Q - 1);
                from = pv_formant_m(c, tf, phi, D, s, first) - W - 1;
                to = pv_formant_m(c, tf, phi, D, s, last) + W + 1;
            }
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

// src0 as the kernel gets it: its low 32 bits.  t < 2^30 and |D| < 2^30 give -2^30 < t - D < 2^31 - 1, and a range begins at most 2 max_period + 65 below
// that, so src0 > -2^31.  A tile that begins past the centre of a compressed grain with D near -2^30 on outputs near 2^30 can have src0 up to 2 max_period
// above 2^31 - 1: such a range lies wholly past the input and holds zeros at every index, the kernel's index arithmetic wraps the same way, and the wrapped
// origin, near -2^31, stages zeros too.
static inline int32_t pv_formant_src0(int64_t s0) { return (int32_t)(uint32_t)(uint64_t)s0; }
