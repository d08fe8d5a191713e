// pv_psola.h -- host <-> kernel contract of the pitch-synchronous overlap-add path (pv_psola_*, include/phaze_amd.h).
//
// A grain is four int32 {t, tf, dq, L}: a Hann window of half length L samples centred at output position t + tf / 256 (tf in 0 .. 255) over the
// input shifted by dq / 256 samples: output n of the grain reads the input at the real position n - dq / 256.  2 <= L <= max_period <= 4096,
// |dq| <= 256 max_period, centres non-decreasing, positions relative to the buffer and below 2^30.  With Q = 256, for output n and grain g:
//   window   ua = |256 (n - t) - tf|; the weight is 0 when ua >= 256 L.  Else q = (4 ua) div L, rem = (4 ua) mod L (exact, 4 ua < 2^22),
//            f = f32(rem) * (1.0f / f32(L)), h = fmaf(f, Hn[q + 1] - Hn[q], Hn[q]); Hn[q] = f32((1 + cos(pi q / 1024)) / 2), q = 0 .. 1023,
//            Hn[1024] = Hn[1025] = 0.
//   sample   D = dq div 256, phi = dq mod 256 (floored).  phi == 0: xt = x[n - D], the sample itself.  Else theta = 256 - phi, b = n - D - 1, the taps
//            i = 0 .. 63 read x[b - 31 + i] with weight w_i = P[|256 (i - 31) - theta|], P the prototype table of pv_vari.h, entries used as they
//            are; a = s = 0, for i ascending a = fmaf(w_i, x_i, a) and s = s + w_i, then xt = a / s.  x is 0 outside [0, nin).
//   output   num = den = 0; for the grains g ascending with h != 0: num = fmaf(h, xt, num), den = den + h; y[n] = num / den, or 0 where no grain
//            covers n.  A grain whose h is exactly 0 touches neither sum.
// SUMMATION ORDER (part of the contract: any tiling, and so any partition of the output range into calls, gives the same bits): the order is a
// function of (g, i) alone.  NON-FINITE INPUT: y[n] is non-finite exactly when a non-finite sample lies under a tap of a grain with h != 0 (all 64
// taps, or the one sample when phi == 0): every covering grain runs all its taps whatever the tile, so no select on the weight is needed.
//
// One launch covers `nout` outputs of `nch` channels from position out_first on, one workgroup per (tile of PV_PSOLA_TILE consecutive outputs,
// channel).  One grain table serves all channels.  The host uploads the table and per tile the contiguous range [first, end) of grains that can
// overlap it; the kernel rejects the grains of the range that do not cover an output.
// LDS: the tile's input span (positions j0 - max_period - 32 .. j0 + tile + max_period + 31, sample e at word e + (e >> 6) as pv_resample.h, zeros
// outside the input), then P, then Hn.  Every LDS index is clamped: a table that got past validation cannot leave the span.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../resample/pv_vari.h"

#define PV_PSOLA_THREADS 256
#define PV_PSOLA_R 4                                   // outputs per thread, PV_PSOLA_THREADS apart
#define PV_PSOLA_TILE (PV_PSOLA_THREADS * PV_PSOLA_R)
#define PV_PSOLA_TAPS 64                               // taps of a fractionally shifted grain
#define PV_PSOLA_Q 256                                 // positions per sample
#define PV_PSOLA_WINDOW 1026                           // Hn[0 .. 1023] and two zero entries
#define PV_PSOLA_WINDOW_WORDS ((PV_PSOLA_WINDOW + 3) & ~3)
#define PV_PSOLA_MAX_PERIOD 4096
#define PV_PSOLA_MAX_POSITION (1 << 30)

struct PvPsolaParams {
    const float *in;           // [nch][in_stride]; in[0] is the sample at buffer position in_first, in_count samples are there (zero elsewhere)
    float *out;                // [nch][out_stride]; out[0] is output out_first
    const float *ptable;       // P, PV_VARI_TABLE_WORDS floats, 16-byte aligned
    const float *htable;       // Hn, PV_PSOLA_WINDOW_WORDS floats, 16-byte aligned
    const int4 *grains;        // {t, tf, dq, L}
    const int2 *tile_grains;   // [tiles]: the grains [x, y) that can overlap the tile
    long in_stride, out_stride;
    int in_first, in_count;
    int out_first, nout, nch;
    int max_period;
    int span;                  // staged samples per tile: PV_PSOLA_TILE + 2 max_period + PV_PSOLA_TAPS
};

static inline __host__ __device__ int pv_psola_span(int max_period) { return PV_PSOLA_TILE + 2 * max_period + PV_PSOLA_TAPS; }
static inline __host__ __device__ size_t pv_psola_span_words(int span) { return ((size_t)span + ((size_t)span >> 6) + 4) & ~(size_t)3; }
// dynamic LDS of a launch
static inline size_t pv_psola_lds_bytes(int max_period)
{
    return 4 * (pv_psola_span_words(pv_psola_span(max_period)) + PV_VARI_TABLE_WORDS + PV_PSOLA_WINDOW_WORDS);
}

// Asynchronous on `stream`.
hipError_t pv_launch_psola(const PvPsolaParams &p, hipStream_t stream);
