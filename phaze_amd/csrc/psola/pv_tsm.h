// pv_tsm.h -- host <-> kernel contract of time-scale modification on the overlap-add path (pv_tsm_*, include/phaze_amd.h).
//
// A far grain is four int32 {t, w, D, L} with w = tf + 256 phi, tf and phi in 0 .. 255: a Hann window of half length L samples centred at output
// position t + tf / 256 over the input displaced by D + phi / 256 samples: output n of the grain reads the input at the real position
// n - D - phi / 256.  2 <= L <= max_period <= 4096, |D| < 2^30, centres non-decreasing, positions relative to the buffer and below 2^30.  D is the
// `dq div 256` of pv_psola.h and phi its `dq mod 256`; everything else is pv_psola.h word for word.  With Q = 256, for output n and grain g:
//   window   ua = |256 (n - t) - tf|; the weight is 0 when ua >= 256 L.  Else q = (4 ua) div L, rem = (4 ua) mod L (exact, 4 ua < 2^22),
//            f = f32(rem) * (1.0f / f32(L)), h = fmaf(f, Hn[q + 1] - Hn[q], Hn[q]); Hn the table of pv_psola_window.
//   sample   phi == 0: xt = x[n - D], the sample itself.  Else theta = 256 - phi, b = n - D - 1, the taps i = 0 .. 63 read x[b - 31 + i] with weight
//            w_i = P[|256 (i - 31) - theta|], P the prototype table of pv_vari.h, entries used as they are; a = s = 0, for i ascending
//            a = fmaf(w_i, x_i, a) and s = s + w_i, then xt = a / s.  x is 0 outside [0, nin).
//   output   num = den = 0; for the grains g ascending with h != 0: num = fmaf(h, xt, num), den = den + h; y[n] = num / den, or 0 where no grain
//            covers n.  A grain whose h is exactly 0 touches neither sum.
// So a table whose grains all have |256 D + phi| <= 256 max_period is pv_psola_process's input in another notation, and the kernel gives its bits.
// SUMMATION ORDER (part of the contract: any tiling, and so any partition of the output range into calls, gives the same bits): the order is a
// function of (g, i) alone.  NON-FINITE INPUT: as pv_psola.h.
//
// One launch covers `nout` outputs of `nch` channels from position out_first on, one workgroup per (tile of PV_TSM_TILE consecutive outputs,
// channel).  One grain table serves all channels.  Per tile [j0, j1) the host uploads one int4 {g_first, g_end, src0, src_count}: the contiguous
// range of grains that can overlap the tile (pv_psola_capi.hip's walk) and the source range those grains read inside the tile,
//   lo = min (max(j0, t - L) - D - 33),  hi = max (min(j1, t + L) - D + 32)  over the grains of the range with t + L >= j0 and t - L < j1,
// src0 = lo, src_count = hi - lo (every tap of a covered output lies in [lo + 1, hi - 1]); {a, b, 0, 0} for a tile no grain reaches.  The host
// refuses a call with a tile whose src_count exceeds span(max_period, max_rate) = max_rate (PV_TSM_TILE + 2 max_period) + 4 max_period + 64.
// LDS: the tile's source range (sample e = buffer position src0 + e at word e + (e >> 6) as pv_resample.h, zeros outside the input), then P, then
// Hn.  Every LDS index is clamped: a table that got past validation cannot leave the span.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../resample/pv_vari.h"

#define PV_TSM_THREADS 256
#define PV_TSM_R 4                                     // outputs per thread, PV_TSM_THREADS apart
#define PV_TSM_TILE (PV_TSM_THREADS * PV_TSM_R)
#define PV_TSM_TAPS 64                                 // taps of a fractionally displaced grain
#define PV_TSM_Q 256                                   // positions per sample
#define PV_TSM_WINDOW 1026                             // Hn[0 .. 1023] and two zero entries
#define PV_TSM_WINDOW_WORDS ((PV_TSM_WINDOW + 3) & ~3)
#define PV_TSM_MAX_PERIOD 4096
#define PV_TSM_MAX_RATE 4
#define PV_TSM_MAX_POSITION (1 << 30)
#define PV_TSM_LDS_BYTES (160 * 1024)                  // LDS of a compute unit of gfx950: what one workgroup may have

struct PvTsmParams {
    const float *in;           // [nch][in_stride]; in[0] is the sample at buffer position in_first, in_count samples are there (zero elsewhere)
    float *out;                // [nch][out_stride]; out[0] is output out_first
    const float *ptable;       // P, PV_VARI_TABLE_WORDS floats, 16-byte aligned
    const float *htable;       // Hn, PV_TSM_WINDOW_WORDS floats, 16-byte aligned
    const int4 *grains;        // {t, w, D, L}
    const int4 *tiles;         // [tiles]: {g_first, g_end, src0, src_count}
    long in_stride, out_stride;
    long long in_first, in_count;
    int out_first, nout, nch;
    int span;                  // staged samples per tile at most: pv_tsm_span(max_period, max_rate)
};

static inline __host__ __device__ int pv_tsm_span(int max_period, int max_rate) { return max_rate * (PV_TSM_TILE + 2 * max_period) + 4 * max_period + PV_TSM_TAPS; }
static inline __host__ __device__ size_t pv_tsm_span_words(int span) { return ((size_t)span + ((size_t)span >> 6) + 4) & ~(size_t)3; }
// dynamic LDS of a launch
static inline size_t pv_tsm_lds_bytes(int span) { return 4 * (pv_tsm_span_words(span) + PV_VARI_TABLE_WORDS + PV_TSM_WINDOW_WORDS); }

// Asynchronous on `stream`.
hipError_t pv_launch_tsm(const PvTsmParams &p, hipStream_t stream);
