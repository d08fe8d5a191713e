// pv_epoch.h -- host <-> kernel contract of the epoch records (pv_epoch_*, include/phaze_amd.h): where in a frame the pitch pulses sit.
//
// One workgroup per (frame, channel).  Frame m reads x[m hop, m hop + window) and the one int32 p = periods[m], the period in 1/256 sample (one row
// for all channels); there is no padding and no state.  The record is four int32 {pos, K, w, s}, an exact integer function of (frame, p):
//   scale    A = max |x| (as pv_f0_kernels.hip, one bit narrower): A = f 2^e, f in [0.5, 1), q_i = rint(ldexpf(x_i, 10 - e)), |q_i| <= 1024.  Silence, a
//            non-finite sample or a p outside [256 * 8, 256 max_period] give {0, 0, 0, 0}.
//   sizes    w = max(2, p >> 10), Pc = (p + 255) >> 8, S(a, b) = sum_{a <= i < b} q_i^2
//   rise     D[n] = S(n, n + w) - S(n - w, n), mass M[n] = S(n - w, n + w), for w <= n <= window - w (a window sum is at most 2^30)
//   comb     K = #{k >= 0: w + Pc - 1 + ((k p) >> 8) <= window - w}, C(phi) = sum_{k < K} D[w + phi + ((k p) >> 8)] in int64, phi = 0 .. Pc - 1
//   record   {w + phi*, K, w, (max(C(phi*), 0) 2^14) div Mtot}, phi* the first argmax, Mtot = sum_{k < K} M[w + phi* + ((k p) >> 8)], 0 when Mtot == 0
// LDS: cs[i] = S(0, i) for i = 0 .. window as wrapping uint32 (every difference used is below 2^31), then the words of the workgroup reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PV_EPOCH_THREADS 256
#define PV_EPOCH_MIN_PERIOD 8
#define PV_EPOCH_MAX_PERIOD 2048
#define PV_EPOCH_MAX_WINDOW 8192
#define PV_EPOCH_MAX_HOP 4096
#define PV_EPOCH_RED_WORDS 16                          // 4 x uint32, 4 x int64, 4 x int32

struct PvEpochParams {
    const float *in;           // channel c at in + c * in_stride: (nframes - 1) hop + window samples
    long in_stride;
    const int *periods;        // [nframes], in 1/256 sample
    int4 *rec;                 // channel c at rec + c * rec_stride: nframes records
    long rec_stride;
    int window, hop, max_period;
};

static inline __host__ __device__ int pv_epoch_prefix_words(int window) { return (window + 1 + 3) & ~3; }
// dynamic LDS of a launch
static inline size_t pv_epoch_lds_bytes(int window) { return 4 * ((size_t)pv_epoch_prefix_words(window) + PV_EPOCH_RED_WORDS); }

// Asynchronous on `stream`.
hipError_t pv_launch_epoch(const float *in, long in_stride, int nch, int nframes, int window, int hop, int max_period, const int *periods, int *records,
                           long rec_stride, hipStream_t stream);
