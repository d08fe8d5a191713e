// pv_contour_kernels.hip -- the candidate table of the pitch contour tracker (pv_contour_track), gfx950: the K best dips of YIN's c curve.
//
// One workgroup per (frame, channel); the contract is pv_contour.h.  The scale, the lag products and the two scans restate pv_f0_kernels.hip (that file is
// pinned by its own tests and stays as it is): P[n] = {q_n, q_{n+1}} as packed int16 pairs, A2[k] = {q_2k, q_2k+1} cut off at W, dd[tau] int64: r, then d
// in place, cc[tau] int32; a thread owns four consecutive lags and slides a window of eight words of P over the frame, and an int32 partial holds 256
// products before it is widened.  What is new is the last step: once cum is formed dd is dead, so the key of every dip goes there (NONE for a lag that is
// no dip) and K rounds of the workgroup's 64-bit min-reduction, each over the keys strictly above the one taken before, give the table in key order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_contour.h"
#include "pv_stretch.h"

namespace {

constexpr int CT_TPB = PV_CONTOUR_THREADS;
constexpr int CT_WAVES = CT_TPB / 64;
constexpr int C_ONE = 1 << 14;

typedef short short2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(unsigned a, unsigned b, int c)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), c, false);
}

struct PvContourParams {
    const float *in;          // channel c at in + c * in_stride: (nframes - 1) hop + W + max_lag samples
    long in_stride;
    int4 *cand;               // frame m of channel c at cand + K (c * cand_stride + m): K slots
    long cand_stride;
    int W, hop, min_lag, max_lag, K, bias;
    int n_p, n_a;             // words of P (a multiple of 4, >= round4(W) + max_lag + 8) and of A2 (round4(W) / 2)
    int n_d;                  // entries of dd and cc (max_lag + 4)
};

__device__ __forceinline__ unsigned block_umax(unsigned v, unsigned *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned r = red[0];
#pragma unroll
    for (int w = 1; w < CT_WAVES; w++) r = max(r, red[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ long long block_min64(long long v, long long *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = red[0];
#pragma unroll
    for (int w = 1; w < CT_WAVES; w++) r = min(r, red[w]);
    __syncthreads();
    return r;
}

// the sum of v over the threads before this one
__device__ __forceinline__ long long block_exclusive_sum(long long v, long long *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = __shfl_up(s, off);
        if (lane >= off) s += o;
    }
    if (lane == 63) red[wave] = s;
    __syncthreads();
    long long base = 0;
#pragma unroll
    for (int w = 0; w < CT_WAVES - 1; w++)
        if (w < wave) base += red[w];
    __syncthreads();
    return base + s - v;
}

__global__ __launch_bounds__(CT_TPB) void pv_contour_kernel(PvContourParams p)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ unsigned redu[CT_WAVES];
    __shared__ long long redl[CT_WAVES];
    unsigned *P = (unsigned *)lds;
    unsigned *A2 = P + p.n_p;
    long long *dd = (long long *)(A2 + p.n_a);                        // n_p and n_a are even: 8-byte aligned
    int *cc = (int *)(dd + p.n_d);
    const int tid = threadIdx.x;
    const int W = p.W, ML = p.max_lag, L = W + ML, K = p.K;
    const float *x = p.in + (long)blockIdx.y * p.in_stride + (long)blockIdx.x * p.hop;
    int4 *slot = p.cand + ((long)blockIdx.y * p.cand_stride + blockIdx.x) * K + tid;      // thread k < K writes slot k

    // ---- scale -------------------------------------------------------------------------------------------------------------------------
    unsigned amax = 0;
    for (int n = tid; n < L; n += CT_TPB) amax = max(amax, __float_as_uint(x[n]) & 0x7fffffffu);
    amax = block_umax(amax, redu);
    if (amax == 0 || amax >= 0x7f800000u) {                              // silence, or a sample that is not finite
        if (tid < K) *slot = int4{0, 0, 0, 0};
        return;
    }
    const int ef = (int)(amax >> 23);
    const int e = ef ? ef - 126 : -117 - __clz(amax);                    // A = f 2^e, f in [0.5, 1); a subnormal A = m 2^-149 has e = (32 - clz m) - 149
    const int sh = 11 - e;
    for (int n = tid; n < p.n_p; n += CT_TPB) {
        const int q0 = n < L ? (int)rintf(ldexpf(x[n], sh)) : 0;
        const int q1 = n + 1 < L ? (int)rintf(ldexpf(x[n + 1], sh)) : 0;
        P[n] = ((unsigned)q0 & 0xffffu) | ((unsigned)q1 << 16);
    }
    __syncthreads();
    for (int k = tid; k < p.n_a; k += CT_TPB) {
        const unsigned w = P[2 * k];
        A2[k] = 2 * k + 1 < W ? w : 2 * k < W ? (w & 0xffffu) : 0u;
    }
    __syncthreads();

    // ---- r(tau), tau = 0 .. max_lag: four lags per thread -------------------------------------------------------------------------------
    const int Wr = 2 * p.n_a;                                             // W rounded up to 4: the pairs beyond W are zero in A2
    for (int t0 = 4 * tid; t0 <= ML; t0 += 4 * CT_TPB) {
        long long r0 = 0, r1 = 0, r2 = 0, r3 = 0;
        const uint4 *Pw = (const uint4 *)(P + t0);                        // t0 and i are multiples of 4: 16-byte aligned
        uint4 lo = Pw[0];
        for (int ib = 0; ib < Wr; ib += 256) {
            const int ie = min(ib + 256, Wr);
            int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int i = ib; i < ie; i += 4) {
                const uint2 a = *(const uint2 *)(A2 + (i >> 1));          // {q_i, q_i+1}, {q_i+2, q_i+3}: the same address in every lane
                const uint4 hi = Pw[(i >> 2) + 1];
                a0 = dot2(a.x, lo.x, a0); a0 = dot2(a.y, lo.z, a0);
                a1 = dot2(a.x, lo.y, a1); a1 = dot2(a.y, lo.w, a1);
                a2 = dot2(a.x, lo.z, a2); a2 = dot2(a.y, hi.x, a2);
                a3 = dot2(a.x, lo.w, a3); a3 = dot2(a.y, hi.y, a3);
                lo = hi;
            }
            r0 += a0; r1 += a1; r2 += a2; r3 += a3;
        }
        dd[t0] = r0; dd[t0 + 1] = r1; dd[t0 + 2] = r2; dd[t0 + 3] = r3;    // t0 + 3 <= max_lag + 3 < n_d
    }
    __syncthreads();

    // ---- d, cum and c: each thread a run of consecutive lags, two workgroup scans ---------------------------------------------------------
    const long long E0 = dd[0];
    const int chunk = (ML + CT_TPB - 1) / CT_TPB;
    const int ta = 1 + tid * chunk, tb = min(ta + chunk, ML + 1);         // this thread's lags [ta, tb)
    long long s = 0;
    for (int t = ta; t < tb; t++) {
        const int u = (short)(P[t - 1 + W] & 0xffffu), v = (short)(P[t - 1] & 0xffffu);
        s += u * u - v * v;
    }
    long long G = block_exclusive_sum(s, redl);
    s = 0;
    for (int t = ta; t < tb; t++) {
        const int u = (short)(P[t - 1 + W] & 0xffffu), v = (short)(P[t - 1] & 0xffffu);
        G += u * u - v * v;
        const long long d = 2 * E0 + G - 2 * dd[t];
        dd[t] = d;
        s += d;
    }
    long long cum = block_exclusive_sum(s, redl);
    for (int t = ta; t < tb; t++) {
        const long long d = dd[t];
        cum += d;
        cc[t] = cum > 0 ? (int)(((unsigned long long)d * (unsigned long long)t << 14) / (unsigned long long)cum) : C_ONE;
    }
    if (tid == 0) cc[0] = C_ONE;
    __syncthreads();

    // ---- the keys of the dips, over d --------------------------------------------------------------------------------------------------------
    constexpr long long NONE = 0x7fffffffffffffffLL;
    const int hiLag = ML - 1;                                             // dips: [min_lag, max_lag - 1]
    for (int t = p.min_lag + tid; t <= hiLag; t += CT_TPB) {
        const int c = cc[t];
        dd[t] = c < cc[t - 1] && c <= cc[t + 1] ? ((long long)(c + p.bias * t / ML) << 16) | t : NONE;      // bias t <= 2^14 4095: an int32
    }
    // a thread reads back only the keys it wrote: no barrier

    // ---- K rounds: the smallest key above the last one taken ---------------------------------------------------------------------------------
    long long last = -1, mine = NONE;
    for (int k = 0; k < K; k++) {
        long long best = NONE;
        for (int t = p.min_lag + tid; t <= hiLag; t += CT_TPB) {
            const long long key = dd[t];
            if (key > last) best = min(best, key);
        }
        best = block_min64(best, redl);
        if (best == NONE) break;                                           // the same in every thread: fewer dips than K
        if (tid == k) mine = best;
        last = best;
    }
    if (tid < K) {
        const int tau = (int)(mine & 0xffff);
        *slot = mine != NONE ? int4{tau, cc[tau - 1], cc[tau], cc[tau + 1]} : int4{0, 0, 0, 0};
    }
}

std::atomic<bool> g_lds_contour[16];

}  // namespace

hipError_t pv_launch_contour(const float *in, long in_stride, int nch, int nframes, int W, int hop, int min_lag, int max_lag, int K, int bias, int *cand,
                             long cand_stride, hipStream_t st)
{
    if (W < 16 || W > 4096 || min_lag < 2 || min_lag >= max_lag || max_lag > 4096 || hop < 1 || hop > 4096 || K < 1 || K > PV_CONTOUR_MAX_CANDIDATES
        || bias < 0 || bias > PV_CONTOUR_MAX_BIAS || nch < 1 || nch > 65535 || nframes < 1 || ((uintptr_t)cand & 15) != 0)
        return hipErrorInvalidValue;
    const int wr = (W + 3) / 4 * 4;
    PvContourParams p{in, in_stride, (int4 *)cand, cand_stride, W, hop, min_lag, max_lag, K, bias, (wr + max_lag + 8 + 3) / 4 * 4, wr / 2, max_lag + 4};
    const hipError_t e = pv_set_dynamic_lds_once(g_lds_contour, (const void *)pv_contour_kernel, (int)pv_f0_lds_bytes(4096, 4096));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pv_contour_kernel, dim3((unsigned)nframes, (unsigned)nch), dim3(CT_TPB), pv_f0_lds_bytes(W, max_lag), st, p);
    return hipGetLastError();
}
