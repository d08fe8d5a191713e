// pv_resample.h -- host <-> kernel contract of the band-limited rational resampler (pv_resample_*, include/phaze_amd.h).
//
// Ratio L / M (output samples per input sample, reduced), half width W, T = 2 W taps per phase.  Output j of the stream sits at input position
// j M / L = n_j + phase_j / L and is  y[j] = sum_{i < T} h[phase_j][i] x[n_j - W + 1 + i].
// SUMMATION ORDER (part of the contract: any tiling gives the same bits): one f32 accumulator, acc = 0, then for i = 0, 1, .. T - 1 in this order
// acc = fmaf(h[phase_j][i], x[n_j - W + 1 + i], acc).  The order is a function of i alone.
// NON-FINITE INPUT: every output runs all T taps, a tap that is 0 included, and fmaf(0, NaN, acc) is NaN: output j is non-finite exactly when one of
// the T samples x[n_j - W + 1 .. n_j + W] is, carried history included.  Which taps run does not depend on the tiling, so this is the same in every
// split of a stream into calls.  (pv_vari.h has the other rule: there a launch may skip zero-weight taps, so such a tap must read nothing.)
//
// One launch covers `nout` outputs of `nch` channels, one workgroup per (tile of `tile` outputs, channel).  Everything the kernel indexes with is
// relative to the call: input index r means in[r] for r >= 0 and hist[T - 1 + r] for r < 0 (the carried newest T - 1 samples).  The host passes the
// position of the call's FIRST output, taken from the stream's int64 counters: phase0 = J0 M mod L and n0 = floor(J0 M / L) - W + 1 - I0, the input
// index of its first tap.  A workgroup advances that pair by tile_index * tile * M in one 64-bit division; everything behind it is 32-bit.
// A thread owns `PV_RESAMPLE_R` outputs `lane_stride` apart.  In the shared form lane_stride is a multiple of L, so the R outputs have ONE tap row,
// read once per tap, and their inputs lie lane_stride M / L apart.
// Device tap table: TRANSPOSED, taps[i * L + phase] (the exported table of pv_resample_design is [phase][i]): the lanes of a wave hold different
// phases, so a row of it is what they read together -- distinct banks in LDS, whole cache lines through L2.
// Staged input in LDS: sample e of the tile's span lives at word e + (e >> 6), one pad word per 64, which spreads the stride-2 / 4 / 8 reads of
// M / L = 2, 4, 8 over all 64 banks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PV_RESAMPLE_THREADS 256
#define PV_RESAMPLE_R 4

struct PvResampleParams {
    const float *in;          // [nch][in_stride], nin new samples per channel
    float *out;               // [nch][out_stride], nout samples per channel
    const float *hist_in;     // [nch][hist_stride], T - 1 samples per channel
    float *hist_out;          // the same slots after the call
    const float *taps;        // [T][L]
    long in_stride, out_stride, hist_stride;
    long long n0;             // input index (relative to in[0]) of the first tap of output 0 of the call
    int phase0;               // phase of output 0 of the call
    int L, M, T;
    int nin, nout, nch;
    int tile;                 // outputs per workgroup = PV_RESAMPLE_R * lane_stride
    int lane_stride;          // shared form: L * floor(threads / L); generic form: threads
    int span;                 // staged input samples per tile: (tile - 1) M / L + 1 + T, rounded up
};

// LDS words of the staged span (with its padding) and of the whole workgroup
static inline __host__ __device__ size_t pv_resample_span_words(int span) { return ((size_t)span + ((size_t)span >> 6) + 4) & ~(size_t)3; }   // a multiple of 4: the taps behind it stay 16-byte aligned
static inline size_t pv_resample_lds_bytes(int span, bool taps_in_lds, int L, int T)
{
    return sizeof(float) * (pv_resample_span_words(span) + (taps_in_lds ? (size_t)L * (size_t)T : 0));
}

// Asynchronous on `stream`.  shared: the taps-in-LDS instance (needs L <= PV_RESAMPLE_THREADS and lane_stride a multiple of L), else the generic one.
hipError_t pv_launch_resample(const PvResampleParams &p, bool shared, hipStream_t stream);
// hist_out[c][e] = the newest T - 1 samples of (hist_in[c] ++ in[c][0 .. nin)), for nch channels.
hipError_t pv_launch_resample_history(const PvResampleParams &p, hipStream_t stream);
