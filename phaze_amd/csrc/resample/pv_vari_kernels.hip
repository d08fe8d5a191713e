// pv_vari_kernels.hip -- variable-ratio band-limited resampler for gfx950: every block of B input samples emits its own number of outputs, the
// weights come from one Kaiser-windowed sinc prototype table by linear interpolation (contract, arithmetic and summation order: pv_vari.h).
//
// One workgroup per (tile of consecutive outputs of the call, channel).  It stages the tile's input span -- carried history first, then the call's
// input -- its slice of the prefix table and the prototype table in LDS, finds the smallest count among its blocks (that fixes the taps that can
// be non-zero anywhere in the tile), then every thread runs R = tile / 256 outputs (PV_VARI_R, or one fewer where the steepest span would not fit: two instances) through the taps, tap
// index ascending.  Per output: a search for its
// block in the LDS slice, three integer divisions (position, the per-tap step of the table index, the index of the first tap), then per tap only
// adds, compares and selects on the index pair, two table reads, one input read and three floating-point operations.
// A tile whose span holds a NaN or an Inf (found while staging) takes a second copy of the tap loops that skips zero-weight taps in the numerator.
// The history roll is pv_resample_history (pv_resample_kernels.hip), launched by the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pv_vari.h"

namespace {

__device__ __forceinline__ int lds_word(int e) { return e + (e >> 6); }

// the weight of table position (q, rem / den): exactly 0 from 32 Q on (P[32 Q] = P[32 Q + 1] = 0)
__device__ __forceinline__ float weight(const float *P, int q, int rem, float inv)
{
    const int qc = min(q, PV_VARI_HALF * PV_VARI_Q);
    const float p0 = P[qc], p1 = P[qc + 1];
    return fmaf((float)rem * inv, p1 - p0, p0);
}

// one tap of the numerator.  A weight of exactly 0 leaves the sum as it is whatever the sample holds (0 * NaN and 0 * Inf are NaN): which zero taps a
// launch runs depends on the tile, so they must not show in the output (pv_vari.h, NON-FINITE INPUT).  GUARD = false is for a tile whose staged span
// holds finite samples only, where the bare multiply-add gives the same bits.
template <bool GUARD>
__device__ __forceinline__ float tap(float w, float x, float num)
{
    return (!GUARD || w != 0.0f) ? fmaf(w, x, num) : num;
}

__device__ __forceinline__ bool non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// the taps of a thread's R outputs, tap index ascending; (q, rem) arrives standing for tap i_lo
template <int R, bool GUARD>
__device__ __forceinline__ void run_taps(const float *P, const float *xs, int i_lo, int W, int i_hi, const int (&off)[R], const float (&inv)[R], const int (&den)[R],
                                         const int (&dq)[R], const int (&dr)[R], int (&q)[R], int (&rem)[R], float (&num)[R], float (&sum)[R])
{
    // taps at or before the output position: a falls by c per tap
    for (int i = i_lo; i < W; i++) {
#pragma unroll
        for (int k = 0; k < R; k++) {
            const float w = weight(P, q[k], rem[k], inv[k]);
            num[k] = tap<GUARD>(w, xs[lds_word(off[k] + i)], num[k]);
            sum[k] += w;
            q[k] -= dq[k]; rem[k] -= dr[k];
            if (rem[k] < 0) { rem[k] += den[k]; q[k] -= 1; }
        }
    }
    // (q, rem) now stands for a Q = (r - c) Q < 0, floored; tap W has a = c - r
#pragma unroll
    for (int k = 0; k < R; k++) {
        q[k] = rem[k] == 0 ? -q[k] : -q[k] - 1;
        rem[k] = rem[k] == 0 ? 0 : den[k] - rem[k];
    }
    // taps behind the output position: a grows by c per tap
    for (int i = W; i <= i_hi; i++) {
#pragma unroll
        for (int k = 0; k < R; k++) {
            const float w = weight(P, q[k], rem[k], inv[k]);
            num[k] = tap<GUARD>(w, xs[lds_word(off[k] + i)], num[k]);
            sum[k] += w;
            q[k] += dq[k]; rem[k] += dr[k];
            if (rem[k] >= den[k]) { rem[k] -= den[k]; q[k] += 1; }
        }
    }
}

template <int R>
__global__ __launch_bounds__(PV_VARI_THREADS) void pv_vari_kernel(PvVariParams p)
{
    extern __shared__ float4 lds4[];
    __shared__ int s_minc, s_bad;                               // the tile's smallest count; whether its span holds a NaN or an Inf
    float *xs = (float *)lds4;
    int *ps = (int *)(xs + pv_vari_span_words(p.span));
    float *P = (float *)(ps + pv_vari_prefix_words(p.tile));
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int B = p.B, W = p.W, T = p.T;
    const int j0 = (int)blockIdx.x * p.tile;
    const int cnt = min(p.tile, p.nout - j0);
    const int2 tb = p.tile_blocks[blockIdx.x];
    const int b0 = tb.x, nb = tb.y - tb.x + 1;                  // 1 <= nb <= tile: every block holds at least one output

    if (tid == 0) { s_minc = 0x7fffffff; s_bad = 0; }
    __syncthreads();
    for (int j = tid; j <= nb; j += PV_VARI_THREADS) {
        const int v = p.prefix[b0 + j];
        ps[j] = v;
        if (j < nb) atomicMin(&s_minc, p.prefix[b0 + j + 1] - v);
    }
    // the tile's first output: block b0, k = j0 - prefix[b0]; (k B) < 2^25
    const int pf0 = p.prefix[b0], c0 = p.prefix[b0 + 1] - pf0;
    const int n_first = b0 * B + (int)((unsigned)((j0 - pf0) * B) / (unsigned)c0);
    const int r0 = n_first - (T - 1);                           // input index of the tile's first tap; >= -(T - 1)

    // ---- stage span samples: e -> input index r0 + e; below 0 history, 0 <= . < nin the call's input, anything else (never needed by a stored output) zero
    const int span = p.span;
    const float *in_c = p.in + (long)ch * p.in_stride;
    const float *hist = p.hist_in + (long)ch * p.hist_stride;
    const int hb = T - 1 + r0;                                  // history index of e = 0
    const int e_in0 = min(span, max(0, -r0));
    const int e_in1 = max(e_in0, min(span, p.nin - r0));
    bool bad = false;
    for (int e = tid; e < e_in0; e += PV_VARI_THREADS) {
        const float v = (hb + e >= 0) ? hist[hb + e] : 0.0f;
        xs[lds_word(e)] = v;
        bad |= non_finite(v);
    }
    for (int e = e_in1 + tid; e < span; e += PV_VARI_THREADS) xs[lds_word(e)] = 0.0f;
    {
        const int mis = (int)((((uintptr_t)in_c >> 2) + (uintptr_t)(long)(r0 + e_in0)) & 3);      // in_c + r0 + e_in0 - mis is 16-byte aligned
        const int base = e_in0 - mis;
        const int quads = (e_in1 - base + 3) >> 2;
        for (int q = tid; q < quads; q += PV_VARI_THREADS) {
            const int e = base + 4 * q;
            if (e >= e_in0 && e + 4 <= e_in1) {
                const float4 v = *(const float4 *)(in_c + (r0 + e));
                xs[lds_word(e)] = v.x; xs[lds_word(e + 1)] = v.y; xs[lds_word(e + 2)] = v.z; xs[lds_word(e + 3)] = v.w;
                bad = bad || non_finite(v.x) || non_finite(v.y) || non_finite(v.z) || non_finite(v.w);
            } else {
                for (int u = 0; u < 4; u++)
                    if (e + u >= e_in0 && e + u < e_in1) {
                        const float v = in_c[r0 + e + u];
                        xs[lds_word(e + u)] = v;
                        bad |= non_finite(v);
                    }
            }
        }
    }
    if (bad) s_bad = 1;                                         // every writer stores the same value
    {
        const float4 *g4 = (const float4 *)p.table;
        for (int k = tid; k < PV_VARI_TABLE_WORDS / 4; k += PV_VARI_THREADS) ((float4 *)P)[k] = g4[k];
    }
    __syncthreads();

    // the taps that can be non-zero somewhere in the tile: i in [W - g, W + g - 1], g = ceil(32 max(B, c) / c) at the tile's smallest c
    const int minc = __builtin_amdgcn_readfirstlane(s_minc);
    const int g = (PV_VARI_HALF * max(B, minc) + minc - 1) / minc;
    const int i_lo = max(0, W - g), i_hi = min(T - 1, W + g - 1);

    float num[R], sum[R], inv[R];
    int q[R], rem[R], dq[R], dr[R], den[R], off[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int j = j0 + min(tid + k * PV_VARI_THREADS, cnt - 1);      // a thread past the tile's end repeats its last output and stores nothing
        int lo = 0, hi = nb - 1;                                         // the last block b with ps[b] <= j
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (ps[mid] <= j) lo = mid; else hi = mid - 1;
        }
        const int c = ps[lo + 1] - ps[lo];
        const unsigned kb = (unsigned)((j - ps[lo]) * B);                // < 2^25
        const unsigned nrel = kb / (unsigned)c;
        const int r = (int)(kb - nrel * (unsigned)c);
        off[k] = min((b0 + lo) * B + (int)nrel - n_first, span - T);     // 0 <= off <= span - T by the span's definition; the clamp keeps a bad table inside LDS
        den[k] = max(B, c);
        inv[k] = 1.0f / (float)den[k];
        const unsigned cq = (unsigned)c * PV_VARI_Q;
        dq[k] = (int)(cq / (unsigned)den[k]);
        dr[k] = (int)(cq - (unsigned)dq[k] * (unsigned)den[k]);
        const unsigned aq = ((unsigned)(W - 1 - i_lo) * (unsigned)c + (unsigned)r) * PV_VARI_Q;      // tap i_lo: a = (W - 1 - i_lo) c + r, a Q < 2^30
        q[k] = (int)(aq / (unsigned)den[k]);
        rem[k] = (int)(aq - (unsigned)q[k] * (unsigned)den[k]);
        num[k] = 0.0f; sum[k] = 0.0f;
    }
    // workgroup-uniform: the select on the weight only where the span holds a sample it matters for
    if (__builtin_amdgcn_readfirstlane(s_bad)) run_taps<R, true>(P, xs, i_lo, W, i_hi, off, inv, den, dq, dr, q, rem, num, sum);
    else run_taps<R, false>(P, xs, i_lo, W, i_hi, off, inv, den, dq, dr, q, rem, num, sum);
    float *out = p.out + (long)ch * p.out_stride + j0;
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int t = tid + k * PV_VARI_THREADS;
        if (t < cnt) out[t] = num[k] / sum[k];
    }
}

}  // namespace

hipError_t pv_launch_vari(const PvVariParams &p, hipStream_t stream)
{
    if (p.nout <= 0 || p.nch <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.nout + p.tile - 1) / p.tile), (unsigned)p.nch);
    const size_t lds = pv_vari_lds_bytes(p.span, p.tile);
    switch (p.tile / PV_VARI_THREADS) {
    case 4: hipLaunchKernelGGL(pv_vari_kernel<4>, grid, dim3(PV_VARI_THREADS), lds, stream, p); break;
    case 3: hipLaunchKernelGGL(pv_vari_kernel<3>, grid, dim3(PV_VARI_THREADS), lds, stream, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
