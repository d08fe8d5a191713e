// pv_contour.h -- host <-> kernel contract of the pitch contour tracker (pv_contour_*, include/phaze_amd.h): the candidate table of a frame.
//
// One workgroup of 256 threads per (frame, channel).  Frame m reads x[m hop, m hop + W + max_lag) and nothing else; there is no state.  The scale, d(tau),
// cum(tau) and c(tau) for tau = 0 .. max_lag are those of the f0 tracker (pv_f0_kernels.hip, DESIGN.md "Pitch tracking"), with the same limits on W, hop and
// the lags.  Then:
//   dip      a lag tau in [min_lag, max_lag - 1] with c(tau) < c(tau - 1) and c(tau) <= c(tau + 1); both neighbours exist (min_lag >= 2, c(max_lag) is computed)
//   key      ((c(tau) + (bias tau) div max_lag) << 16) | tau, bias in [0, 16384]: c <= 2^26 and tau < 2^16, so a key is below 2^43 and no two are equal
//   table    slot k = {tau, c(tau - 1), c(tau), c(tau + 1)} of the dip with the k-th smallest key, k = 0 .. K - 1; {0, 0, 0, 0} beyond the number of dips,
//            and in every slot of a silent frame or of one with a non-finite sample.  1 <= K <= 8.
// Every value is an exact integer function of the frame, whatever the order of the reductions.
// Layout: a slot is four int32 written with one 16-byte store; the K slots of a frame are contiguous and frame m of channel c starts at
// cand + 4 K (c cand_stride + m): cand_stride counts frames.  cand is 16-byte aligned.
// LDS: the dynamic arrays of pv_f0_kernel (pv_f0_lds_bytes of pv_stretch.h); the keys go where d(tau) was, which is dead once cum is formed.
//
// The path through the table (pv_contour_path.hip) is pure host code in int64.  With tau <= 65535, c values >= 0, jump_cost and voicing_cost <= 2^20: the
// largest intermediate of one frame is 2 jump_cost |tau_b - tau_a| < 2^38, a frame adds less than 2^22 to the cost of a path, and the cost of a path over
// 2^31 - 1 frames stays below 2^53 < 2^62.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PV_CONTOUR_THREADS 256
#define PV_CONTOUR_MAX_CANDIDATES 8
#define PV_CONTOUR_MAX_BIAS 16384

// Asynchronous on `stream`.  Validates as pv_launch_f0 does (hipErrorInvalidValue), and 1 <= K <= 8, 0 <= bias <= 16384, cand 16-byte aligned.
hipError_t pv_launch_contour(const float *in, long in_stride, int nch, int nframes, int W, int hop, int min_lag, int max_lag, int K, int bias, int *cand,
                             long cand_stride, hipStream_t stream);
