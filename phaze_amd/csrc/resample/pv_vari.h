// pv_vari.h -- host <-> kernel contract of the variable-ratio band-limited resampler (pv_vari_*, include/phaze_amd.h).
//
// Block size B, counts within [min_count, max_count], half width W = ceil(32 max(1, B / min_count)), T = 2 W taps.  Block b of the stream takes B input
// samples and emits c = counts[b] outputs; output k of it sits at input position b B + k B / c - W.  With n = b B + (k B) div c and r = (k B) mod c
// tap i reads x[n - 2 W + 1 + i] and lies a = |(i - W + 1) c - r| / c samples from the output position.  den = max(B, c), Q = 256:
//     q = (a Q) div den,  rem = (a Q) mod den,  f = f32(rem) * (1.0f / f32(den)),  w_i = fmaf(f, P[q + 1] - P[q], P[q])   (0 when q >= 32 Q)
//     y = (sum_i w_i x_i) / (sum_i w_i)
// SUMMATION ORDER (part of the contract: any tiling gives the same bits): num = den_sum = 0, then for i ascending num = fmaf(w_i, x_i, num) and
// den_sum = den_sum + w_i, then one IEEE f32 division.  A tap whose weight is exactly 0 leaves both sums as they are, so a launch may skip the taps
// that are 0 for every output of a tile: only i in [W - g, W + g - 1], g = ceil(32 den / c), can be non-zero.
// NON-FINITE INPUT (part of the contract for the same reason: any tiling, and so any split of a stream into calls, gives the same bits).  A tap whose
// weight is exactly 0 does not touch num WHATEVER its sample holds: fmaf(0, NaN, num) and fmaf(0, Inf, num) are NaN, so a tile whose staged span
// holds a non-finite sample selects on w != 0 instead of relying on the product (a clean span keeps the bare multiply-add: the same bits).  Hence: output j is non-finite exactly when a non-finite input sample, carried history included, lies under a
// tap of j whose weight w_i, in the arithmetic above, is non-zero; every other output has the value it would have with those samples replaced by 0.
// (pv_resample.h has the other rule: it runs all T taps of a phase row for every output, zero ones included.)
// (q, rem) is formed incrementally: a Q moves by c Q per tap, so the pair moves by (c Q div den, c Q mod den) with a carry; exact integers, a Q < 2^30.
//
// One launch covers `nout` outputs of `nch` channels, one workgroup per (tile of `tile` consecutive outputs of the call, channel).  Everything the
// kernel indexes with is relative to the call: input index e means in[e] for e >= 0 and hist[T - 1 + e] for e < 0 (the carried newest T - 1 samples).
// The host uploads prefix[0 .. nblocks] (prefix sums of the call's counts, int32) and per tile the blocks that hold its first and its last output.
// LDS: the staged span (sample e at word e + (e >> 6), as pv_resample.h), then the tile's slice of the prefix table, then P.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PV_VARI_THREADS 256
#define PV_VARI_R 4                              // most outputs per thread (PV_VARI_THREADS apart): tile = PV_VARI_THREADS * R, R = PV_VARI_R or PV_VARI_R - 1
#define PV_VARI_Q 256                            // table entries per input sample
#define PV_VARI_HALF 32                          // half width of the prototype in samples
#define PV_VARI_TABLE (PV_VARI_HALF * PV_VARI_Q + 2)     // P[0 .. 32 Q] and one guard entry: 8194 floats, P[32 Q] = P[32 Q + 1] = 0
#define PV_VARI_TABLE_WORDS ((PV_VARI_TABLE + 3) & ~3)

struct PvVariParams {
    const float *in;          // [nch][in_stride], nblocks * B new samples per channel
    float *out;               // [nch][out_stride], nout samples per channel
    const float *hist_in;     // [nch][hist_stride], T - 1 samples per channel
    const float *table;       // P, PV_VARI_TABLE_WORDS floats, 16-byte aligned
    const int *prefix;        // [nblocks + 1]
    const int2 *tile_blocks;  // [tiles]: (block of the tile's first output, block of its last)
    long in_stride, out_stride, hist_stride;
    int B, W, T;
    int nin, nout, nch;       // nin = nblocks * B
    int tile;                 // outputs per workgroup: PV_VARI_THREADS * R, R = PV_VARI_R, or PV_VARI_R - 1 where B / min_count is above 6.4 (pv_vari_lds_bytes)
    int span;                 // staged input samples per tile: floor((tile - 1) B / min_count) + 1 + T
};

static inline __host__ __device__ size_t pv_vari_span_words(int span) { return ((size_t)span + ((size_t)span >> 6) + 4) & ~(size_t)3; }
// the tile's slice of the prefix table: at most tile blocks and one more entry
static inline __host__ __device__ size_t pv_vari_prefix_words(int tile) { return ((size_t)tile + 1 + 3) & ~(size_t)3; }
// dynamic LDS of a launch; the kernel has 16 bytes of static LDS besides
static inline size_t pv_vari_lds_bytes(int span, int tile) { return 4 * (pv_vari_span_words(span) + pv_vari_prefix_words(tile) + PV_VARI_TABLE_WORDS); }

// Asynchronous on `stream`.
hipError_t pv_launch_vari(const PvVariParams &p, hipStream_t stream);
