// pv_takes.h -- host <-> kernel contract of per-take plans on the overlap-add path (pv_takes_*, include/phaze_amd.h): one launch whose tiles belong to
// different takes, each with its own input, grain table, length and output range.
//
// A take is one monophonic recording with its own plan.  Take k's output is exactly what pv_tsm_process gives for take k alone: the far grain
// {t, w, D, L}, the window, sample and output rules, the tile's grain range and source range {g_first, g_end, src0, src_count} and the LDS layout are
// pv_tsm.h's word for word, and the per-(output, grain, tap) arithmetic is restated operation for operation.  SUMMATION ORDER: a function of (g, i)
// alone, so any partition of a take's output range into takes gives the same bits.
//
// What a call uploads (one table, one copy):
//   grains   the takes' tables one after the other, int4 {t, w, D, L}
//   tiles    per tile two int4: {take, first, g_first, g_end} and {src0, src_count, count, 0}.  `take` indexes the take records; `first` is the tile's
//            first output relative to the record's out_first and `count` how many outputs it has (1 .. PV_TSM_TILE); g_first and g_end index the
//            concatenated table
//   order    tile ids: workgroup x of a launch runs tile order[x].  The host sorts the ids by occupancy class (below), (take, tile) order kept within
//            a class, and issues one launch per non-empty class
//   takes    PvTakeRec per take (the host form: per take and piece, with the staged pointers)
// Every index is clamped: the tile id to the call's tile count, the take to the record count, the grain range to the table, every LDS index to the
// staged count.  A table that got past validation cannot leave its buffers.
//
// OCCUPANCY CLASSES.  A launch's dynamic LDS is sized by the longest source range among ITS tiles.  So that one take at a high rate does not put every
// tile of the call at one workgroup per compute unit, a tile has the class
//   cls = min(4, PV_TSM_LDS_BYTES div pv_tsm_lds_bytes(s)),   s = max(128, src_count rounded up to 64)
// (how many such workgroups the LDS of a compute unit holds; P and Hn alone take 36.9 KB, so four is the ceiling), and a launch holds one class.  Where
// the rounded s would not fit the LDS at all (a count within 63 samples of the largest span that fits), s is the count itself and the class is 1.  The
// class groups launches only: the bits do not depend on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pv_tsm.h"

#define PV_TAKES_MAX_TAKES 65536
#define PV_TAKES_CLASSES 4
#define PV_TAKES_TILE_WORDS 8                          // int32 per tile record
#define PV_TAKES_REC_WORDS 16                          // int32 per take record

struct PvTakeRec {
    const float *in;           // channel c at in + c * in_stride; in[0] is the sample at buffer position in_first, in_count samples are there
    float *out;                // channel c at out + c * out_stride; out[0] is output out_first
    long long in_stride, out_stride;
    long long in_first, in_count;
    int out_first;
    int pad[3];
};
static_assert(sizeof(PvTakeRec) == 4 * PV_TAKES_REC_WORDS, "a take record is 16 words");

struct PvTakesParams {
    const float *ptable;       // P, PV_VARI_TABLE_WORDS floats, 16-byte aligned
    const float *htable;       // Hn, PV_TSM_WINDOW_WORDS floats, 16-byte aligned
    const int4 *grains;        // [ngrains]
    const int4 *tiles;         // [ntiles][2]
    const int *order;          // [count]: the launch's tile ids
    const PvTakeRec *takes;    // [ntakes]
    int ngrains, ntiles, ntakes;
    int count;                 // workgroups in x
    int nch;
    int span;                  // staged samples per tile at most in this launch: pv_takes_launch_span of its longest tile, at least 128
};

// Samples the LDS of a launch is sized for when its longest tile reads src_count samples: the count rounded up to 64, at least two tap rows.  A handle's
// span need not be a multiple of 64, so within 63 samples of the largest span that fits the LDS the rounded count would not fit: there the launch is
// sized by the count itself, which fits because the handle's span does (the kernel's layout does not need a multiple of 64).
static inline int pv_takes_launch_span(int src_count)
{
    const int s = (src_count + 63) & ~63;
    if (s < 2 * PV_TSM_TAPS) return 2 * PV_TSM_TAPS;
    return pv_tsm_lds_bytes(s) > PV_TSM_LDS_BYTES ? src_count : s;
}
// 1 .. PV_TAKES_CLASSES for every count a handle accepts
static inline int pv_takes_class(int src_count)
{
    const size_t per = (size_t)PV_TSM_LDS_BYTES / pv_tsm_lds_bytes(pv_takes_launch_span(src_count));
    return per > PV_TAKES_CLASSES ? PV_TAKES_CLASSES : per < 1 ? 1 : (int)per;
}

// Asynchronous on `stream`.
hipError_t pv_launch_takes(const PvTakesParams &p, hipStream_t stream);
