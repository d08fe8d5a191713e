// pv_choir.h -- host <-> kernel contract of full-grain harmony voices on the overlap-add path (pv_choir_*, include/phaze_amd.h): V differently planned
// copies of one input, each overlap-added on its own from grains that may be mirrored, warped or both, summed into one output.
//
// THE GRAIN WORD.  A grain is four int32 {t, w, D, L} with w = tf + 256 phi + 65536 m + 131072 z, 0 <= w < 2^27, tf and phi in 0 .. 255.  m, bit 16, is
// pv_mirror.h's direction bit.  z, bits 17 .. 26, is pv_formant.h's step s in 1/256 under that header's rules: z = 0 means s = 256, else 128 <= z <= 512 and
// s = z; z = 256 is legal and is treated exactly as z = 0.  t, L and the ordering are pv_tsm.h's: 0 <= t < 2^30, 2 <= L <= max_period <= 4096, centres
// non-decreasing on 256 t + tf.  D follows pv_mirror.h: D > -2^30 always, and D < 2^30 only for a forward grain (a mirrored D is a sum of two positions
// below 2^30: any larger int32 is allowed).  A grain is refused for its centre, its length, its shift, its order or its step (the enum below); a step is
// bad when w < 0 or w >= 2^27 or z lies in 1 .. 127 or above 512.
//
// FOUR KINDS OF GRAIN, chosen by (m, s), which are read with the record and so are the same for every lane:
//   m = 0, s = 256   pv_tsm.h's far grain, word for word: output n reads the real position n - D - phi / 256.
//   m = 1, s = 256   pv_mirror.h's mirrored grain, word for word: output n reads D - n - phi / 256.
//   m = 0, s != 256  pv_formant.h's warped grain, word for word: output n reads (t + tf / 256 - D - phi / 256) + (s / 256) (n - t - tf / 256).
//   m = 1, s != 256  new, MIRRORED AND WARPED: output n reads (D - t - tf / 256 - phi / 256) - (s / 256) (n - t - tf / 256): the position the mirrored
//                    grain reads at its centre, and from there s / 256 input samples DOWNWARDS per output sample.  In exact integers:
//                      u = 256 (n - t) - tf (|u| < 2^20 for a covered output, so |s u| < 2^29); v = -256 (tf + phi) - s u in int32;
//                      mm = (D - t) + floor(v / 65536), formed in wrapping unsigned arithmetic as pv_mirror_kernel forms its index; r = v mod 65536 in
//                      0 .. 65535.  The position is mm + r / 65536.
//                    From (mm, r) on the sample rule is pv_formant.h's, unchanged: den = max(256, s); W = 32 for s <= 256 and 64 otherwise; tap
//                    i = 0 .. 2 W - 1 reads x[mm - W + 1 + i] and lies d / 65536 samples from the position, d = |(i - W + 1) 65536 - r|; q = d div den,
//                    rem = d mod den; w_i = 0 when q >= 32 * 256, else f = f32(rem) * (1.0f / f32(den)) and w_i = fmaf(f, P[q + 1] - P[q], P[q]);
//                    a = sum = 0, for i ascending a = fmaf(w_i, x_i, a) and sum = sum + w_i, xt = a / sum; a tap whose weight is exactly 0 touches neither
//                    sum whatever its sample holds, so a launch may skip the taps outside -K <= i - W + 1 <= K + 1, K = ceil(den / 8) - 1.
//                    At s = 256 this rule lands on pv_mirror.h's positions and weights (mm = D - n - 1 and r = 256 (256 - phi) for phi != 0, mm = D - n and
//                    r = 0 for phi == 0; then rem = 0 and q = |256 (i - 31) - theta|): that is why the kinds may share a table, as pv_formant.h argues
//                    for its own case.
//   window, num / den in grain order, the zero weight rule and x = 0 outside [0, nin): pv_tsm.h's, for every kind.
//
// THE MIX is pv_harmony.h's, word for word.  A call has V voices, 1 <= V <= PV_CHOIR_MAX_VOICES; y_v[n] is one num / den over voice v's own grains.
// gains[v nch + c] is a finite float.  For channel c and output n: acc = 0.0f; for v ascending: skip voice v when gains[v nch + c] == 0 or no grain of voice v
// covers n with h != 0 (a skipped voice touches nothing: a NaN under the taps of a muted voice stays out); else acc = acc + mul_rounded(gain, y_v[n]): the
// product rounded to f32 as an operation of its own (pv_mul_rounded.h), then a plain add; never an fmaf.  out[c][n] = acc, exactly 0 where no voice
// contributes.  SUMMATION ORDER: the order of every sum is a function of (v, g, i) alone, so any tiling, and any partition of the output range into
// calls, gives the same bits.  NON-FINITE INPUT: as pv_tsm.h, per voice that is not skipped.
//
// TILES AND THE HULL.  One workgroup per (tile of PV_TSM_TILE outputs, channel).  Per voice the grain range of a tile [j0, j1) is pv_tsm's walk on the
// voice's own table (t and L only).  The source range [lo, hi) of a grain that reaches the tile, with first = max(j0, t - L) and last = min(j1, t + L):
//   m = 0, s = 256   lo = first - D - 33,       hi = last - D + 32                                  (pv_tsm.h)
//   m = 1, s = 256   lo = D - last - 33,        hi = D - first + 32                                 (pv_mirror.h)
//   m = 0, s != 256  lo = M(first) - W - 1,     hi = M(last) + W + 1                                (pv_formant.h; M(n) the m of output n)
//   m = 1, s != 256  lo = M'(last) - W - 1,     hi = M'(first) + W + 1, with
//                    M'(n) = (D - t) + floor((-256 (tf + phi) - s (256 (n - t) - tf)) / 65536), the mm of output n.
// Why every tap of a covered output of a mirrored warped grain lies in [lo + 2, hi - 1]: a covered output n of the tile has first <= n <= last
// (pv_mirror.h: ua < 256 L gives t - L < n <= t + L, and j0 <= n < j1).  The numerator of M' falls by 256 s > 0 per output and floor is monotone, so M'
// does not increase with n: M'(last) <= M'(n) <= M'(first).  The taps of n are M'(n) - W + 1 .. M'(n) + W: the lowest is at least
// M'(last) - W + 1 = lo + 2 and the highest at most M'(first) + W = hi - 1.  This is pv_formant.h's derivation with the two ends swapped, as pv_mirror.h's
// is pv_tsm.h's with the ends swapped.
// A voice's range on a tile is the hull of its grains' ranges; the tile stages the HULL over the voices (voices with no grain on the tile left out), once
// for all of them: src0 = min lo, src_count = max hi - min lo, {0, 0} when no voice has a grain.  The uploaded buffer is pv_harmony.h's, in 32-bit words:
// the grains (4 ngrains, at least 4), the tiles (int2 {src0, src_count} per tile), the ranges (int2 {g_first, g_end} per (tile, voice), indices into the
// concatenated table), the gains (V nch floats).
//
// SPAN.  pv_choir_span(max_period, max_rate) = pv_formant.h's max_rate (PV_TSM_TILE + 2 max_period) + 6 max_period + 192, with its LDS rule: max_period up
// to 3753 at max_rate 1, 2900 at 2, 2331 at 3 and 1925 at 4; pv_choir_create returns PV_ERR_UNSUPPORTED beyond.  The host refuses a call with a tile whose
// hull exceeds the span, before any device work; a hull is never clipped.  Why planned tables keep to it: a grain of pv_choir_plan that is mirrored and
// warped reads (s / 256) L to either side of the same analysis mark A as the forward warped grain would (its centre reads A), so pv_formant.h's budget
// holds per voice; voices planned on one row of rates share the read position, so the marks of all voices on a tile lie in the one range that budget
// allows a single voice (pv_harmony.h's argument).  tests/test_choir_model.py sweeps the corners.
// LDS: pv_tsm.h's layout (the padded span, then P, then Hn), the hull in the place of the source range.  Every LDS index is clamped to the staged count,
// in both directions; the tap base is clamped to [0, sc - 2 W].  Grain records, ranges and gains are read at uniform indices.
//
// Validation, the tile walk and src0 are inline host functions here, so that the handle (pv_choir_capi.hip) and a host-only build share one text.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "pv_tsm.h"

#define PV_CHOIR_MAX_VOICES 8
#define PV_CHOIR_MIRROR_BIT (PV_TSM_Q * PV_TSM_Q)      // bit 16 of w
#define PV_CHOIR_STEP_SHIFT 17                         // z = (w >> 17) & 1023
#define PV_CHOIR_W_END (1 << 27)
#define PV_CHOIR_MIN_STEP 128
#define PV_CHOIR_MAX_STEP 512
#define PV_CHOIR_TAPS 128                              // taps of a warped grain at most (s > 256); 64 for s < 256

struct PvChoirParams {
    const float *in;           // [nch][in_stride]; in[0] is the sample at buffer position in_first, in_count samples are there (zero elsewhere)
    float *out;                // [nch][out_stride]; out[0] is output out_first
    const float *ptable;       // P, PV_VARI_TABLE_WORDS floats, 16-byte aligned
    const float *htable;       // Hn, PV_TSM_WINDOW_WORDS floats, 16-byte aligned
    const int4 *grains;        // {t, w, D, L}, the voices' tables one after the other
    const int2 *tiles;         // [tiles]: {src0, src_count}, the hull
    const int2 *ranges;        // [tiles][nvoices]: {g_first, g_end}
    const float *gains;        // [nvoices][nch]
    long in_stride, out_stride;
    long long in_first, in_count;
    int out_first, nout, nch, nvoices;
    int span;                  // staged samples per tile at most, a multiple of 64 or the handle's span: the longest hull of the launch
};

// Asynchronous on `stream`.
hipError_t pv_launch_choir(const PvChoirParams &p, hipStream_t stream);

// why a grain is refused
enum { PV_CHOIR_BAD_CENTRE = 1, PV_CHOIR_BAD_LENGTH = 2, PV_CHOIR_BAD_SHIFT = 3, PV_CHOIR_BAD_ORDER = 4, PV_CHOIR_BAD_STEP = 5 };

// the step of a valid w: 256 for z = 0
static inline __host__ __device__ int pv_choir_step(int32_t w)
{
    const int z = (w >> PV_CHOIR_STEP_SHIFT) & 1023;
    return z ? z : PV_TSM_Q;
}

static inline __host__ __device__ int pv_choir_span(int max_period, int max_rate) { return max_rate * (PV_TSM_TILE + 2 * max_period) + 6 * max_period + 192; }

// The index of the first grain of ONE voice's table that breaks a rule and *why, or -1.
static inline int64_t pv_choir_check_grains(const int32_t *grains, int64_t ngrains, int max_period, int *why)
{
    long long prev = 0;
    for (int64_t g = 0; g < ngrains; g++) {
        const int32_t t = grains[4 * g], w = grains[4 * g + 1], D = grains[4 * g + 2], L = grains[4 * g + 3];
        int bad = 0;
        const long long c = (long long)t * PV_TSM_Q + (w & (PV_TSM_Q - 1));
        const int z = w >= 0 ? (w >> PV_CHOIR_STEP_SHIFT) : 0;
        if (t < 0 || t >= PV_TSM_MAX_POSITION) bad = PV_CHOIR_BAD_CENTRE;
        else if (w < 0 || w >= PV_CHOIR_W_END || (z != 0 && (z < PV_CHOIR_MIN_STEP || z > PV_CHOIR_MAX_STEP))) bad = PV_CHOIR_BAD_STEP;
        else if (L < 2 || L > max_period) bad = PV_CHOIR_BAD_LENGTH;
        else if (D <= -PV_TSM_MAX_POSITION || (!(w & PV_CHOIR_MIRROR_BIT) && D >= PV_TSM_MAX_POSITION)) bad = PV_CHOIR_BAD_SHIFT;
        else if (c < prev) bad = PV_CHOIR_BAD_ORDER;
        if (bad) {
            if (why) *why = bad;
            return g;
        }
        prev = c;
    }
    return -1;
}

// M(n) of a forward warped grain (mir == 0) or M'(n) of a mirrored warped one, in int64 (the contract above)
static inline long long pv_choir_m(long long t, int tf, int phi, long long D, int s, int mir, long long n)
{
    const long long su = (long long)s * (256LL * (n - t) - tf);
    const long long v = mir ? -256LL * (tf + phi) - su : 256LL * (tf - phi) + su;
    return (mir ? D - t : t - D) + (v >> 16);                           // an arithmetic shift: floor
}

// The tiles of outputs [out_first, out_first + nout) of ONE voice's validated table: tiles[4 k ..] = {g_first, g_end, src0, src_count} of tile k in
// int64, as tests/choir_model.py's tiles().  Returns the number of tiles.  The hull over the voices is the caller's (pv_choir_capi.hip).
static inline int64_t pv_choir_tiles(const int32_t *grains, int64_t ngrains, int max_period, int64_t out_first, int64_t nout, int64_t *tiles)
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
            const int s = pv_choir_step(w), mir = (w & PV_CHOIR_MIRROR_BIT) != 0;
            long long from, to;
            if (s == PV_TSM_Q) {
                from = (mir ? D - last : first - D) - PV_TSM_TAPS / 2 - 1;
                to = (mir ? D - first : last - D) + PV_TSM_TAPS / 2;
            } else {
                const int W = s < PV_TSM_Q ? PV_TSM_TAPS / 2 : PV_CHOIR_TAPS / 2, tf = w & (PV_TSM_Q - 1), phi = (w >> 8) & (PV_TSM_Q - 1);
                from = pv_choir_m(c, tf, phi, D, s, mir, mir ? last : first) - W - 1;
                to = pv_choir_m(c, tf, phi, D, s, mir, mir ? first : last) + W + 1;
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

// src0 as the kernel gets it: its low 32 bits (pv_formant_src0's corner).  A hull the span admits is at most a few ten thousand samples long, so one that
// begins below -2^31 (a mirrored grain with D near -2^30 on outputs near 2^30) or ends above 2^31 - 1 (a mirrored grain with D near 2^31, a compressed
// grain with D near -2^30) lies wholly outside the input, which ends below 2^30: it holds zeros at every index, the kernel's index arithmetic wraps the
// same way, and the wrapped origin stages zeros too.
static inline int32_t pv_choir_src0(int64_t s0) { return (int32_t)(uint32_t)(uint64_t)s0; }
