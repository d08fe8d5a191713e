// pv_harmony.h -- host <-> kernel contract of harmony voices on the overlap-add path (pv_harmony_*, include/phaze_amd.h): V differently planned copies
// of one input, each overlap-added on its own, summed into one output.
//
// A call has V voices, 1 <= V <= PV_HARMONY_MAX_VOICES.  Voice v is a far-grain table in pv_tsm.h's notation and rules, word for word (window, sample,
// num / den in grain order, x = 0 outside the input): y_v[n] is what pv_tsm_process gives for that table alone.  gains[v nch + c] is a finite float per
// (voice, channel).  For channel c and output n:
//   acc = 0.0f; for v ascending: skip voice v when gains[v nch + c] == 0 or no grain of voice v covers n with h != 0 (a skipped voice touches nothing: a
//   NaN under the taps of a muted voice stays out); else acc = acc + mul_rounded(gains[v nch + c], y_v[n]): the product rounded to f32 as an operation of
//   its own (pv_mul_rounded.h), then a plain add; never an fmaf.  out[c][n] = acc, 0 where no voice contributes.
// So numpy float32 reproduces the mix exactly from the per-voice outputs of pv_tsm_process.  One `num / den` per voice: a merged table would normalise
// over all the grains that cover an output and average the voices instead of adding them.
// SUMMATION ORDER (part of the contract: any tiling, and so any partition of the output range into calls, gives the same bits): the order of every sum
// is a function of (v, g, i) alone.  NON-FINITE INPUT: as pv_tsm.h, per voice that is not skipped.
//
// One launch covers `nout` outputs of `nch` channels from position out_first on, one workgroup per (tile of PV_TSM_TILE consecutive outputs, channel).
// The grain tables of the voices are concatenated into one, voice v holding the records [voice_first[v], voice_first[v + 1]).  Per tile [j0, j1) the
// host uploads
//   tiles[tile]              int2 {src0, src_count}: the hull over the voices of pv_tsm.h's per-voice source range [lo_v, hi_v) of the tile,
//                            src0 = min lo_v, src_count = max hi_v - min lo_v, voices with no grain on the tile left out; {0, 0} when no voice has one
//   ranges[tile V + v]       int2 {g_first, g_end}: voice v's contiguous range of grains that can overlap the tile (pv_tsm_capi.hip's walk on the
//                            voice's own table), as indices into the concatenated table
// and per call gains[v nch + c].  The tile's input is staged ONCE for all voices.  The host refuses a call with a tile whose hull exceeds
// pv_tsm_span(max_period, max_rate), even when every voice alone would fit.  The uploaded buffer is, in 32-bit words: the grains (4 ngrains, at least 4),
// the tiles (2 per tile), the ranges (2 V per tile), the gains (V nch floats).
// LDS: pv_tsm.h's, the hull in place of the source range; every LDS index is clamped.  Grain records, ranges and gains are read at uniform indices.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pv_tsm.h"

#define PV_HARMONY_MAX_VOICES 8

struct PvHarmonyParams {
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
    int span;                  // staged samples per tile at most, a multiple of 64: the longest hull of the launch
};

// Asynchronous on `stream`.
hipError_t pv_launch_harmony(const PvHarmonyParams &p, hipStream_t stream);
