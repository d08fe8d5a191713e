// pv_onset_kernels.hip -- onset strength for the time stretch (pv_onset_strength), gfx950, N = 256 .. 8192.
//
// Per group and frame, c_m = #{k in [1, H - 1): mag_m[k] > 4 mag_{m-1}[k] and mag_m[k] > 2^-20 max_k mag_m}, mag the f32 Re^2 + Im^2 of pass B
// (pv_stretch_kernels.hip) on the stretch's own front end (forward<>, MixSrc).  Both factors are powers of two: the comparisons are exact functions
// of mag.  A pure function of its buffer: frames at the fixed hop ha, frame m's window ends at (m + 1) ha, zeros before the buffer, frame -1 all
// zeros, no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_stretch_device.h"

namespace {

// the buffer alone, zeros before it: sample s of the mix of G channels (G = 1: the channel itself)
struct PadSrc {
    MixSrc mix;
    __device__ __forceinline__ float at(long s) const { return s < 0 ? 0.0f : mix.at(s); }
};

constexpr int WAVES = TPB / 64;
constexpr int COUNT_BATCH = TPB;                                      // counts leave the workgroup COUNT_BATCH frames at a time, coalesced

__device__ __forceinline__ float block_max(float v, float *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) r = fmaxf(r, red[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ int block_sum(int v, int *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) r += red[w];
    __syncthreads();
    return r;
}

struct PvOnsetParams {
    const float *in;          // channel c at in + c * in_stride: nframes * ha samples
    long in_stride;
    int *counts;              // group g at counts + g * count_stride: nframes values
    long count_stride;
    int nframes, G, ha, F;    // F: frames per chain
    const double2 *tw64;
    const float *hann;
};

template <int LOG2N>
__global__ __launch_bounds__(TPB) void pv_onset_strength_kernel(PvOnsetParams p)
{
    using C = SC<LOG2N>;
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ float redf[WAVES];
    __shared__ int redi[WAVES];
    __shared__ int batch[COUNT_BATCH];
    double2 *A = (double2 *)lds;
    float *prev = (float *)(lds + C::A_BYTES);
    float *cur = (float *)(lds + C::A_BYTES + C::H4);
    const int j = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const PadSrc src{MixSrc{nullptr, p.in + (long)g * p.G * p.in_stride, 0, 0, p.in_stride, p.G}};
    const int m0 = j * p.F, m1 = min(m0 + p.F, p.nframes);
    if (m0 == 0) {
        for (int k = tid; k < C::H; k += TPB) prev[k] = 0.0f;
    } else {
        forward<LOG2N>(A, src, (long)m0 * p.ha - C::N, p.hann, p.tw64);
        for (int k = tid; k < C::H; k += TPB) {
            const double2 X = A[k];
            prev[k] = (float)__dadd_rn(__dmul_rn(X.x, X.x), __dmul_rn(X.y, X.y));
        }
    }
    __syncthreads();
    int *out = p.counts + (long)g * p.count_stride;
#pragma unroll 1
    for (int m = m0; m < m1; m++) {
        forward<LOG2N>(A, src, (long)(m + 1) * p.ha - C::N, p.hann, p.tw64);
        float mx = 0.0f;
        for (int k = tid; k < C::H; k += TPB) {
            const double2 X = A[k];
            const float v = (float)__dadd_rn(__dmul_rn(X.x, X.x), __dmul_rn(X.y, X.y));
            cur[k] = v;
            mx = fmaxf(mx, v);
        }
        const float floor_v = __fmul_rn(block_max(mx, redf), 0x1p-20f);
        int n = 0;
        for (int k = tid; k < C::H; k += TPB) {
            const float v = cur[k], u = prev[k];
            if (k >= 1 && k < C::H - 1 && v > __fmul_rn(4.0f, u) && v > floor_v) n++;
            prev[k] = v;
        }
        n = block_sum(n, redi);
        const int slot = (m - m0) % COUNT_BATCH;
        if (tid == 0) batch[slot] = n;
        if (slot == COUNT_BATCH - 1 || m == m1 - 1) {
            __syncthreads();
            const int first = m - slot;
            if (tid <= slot) out[first + tid] = batch[tid];
            __syncthreads();
        }
    }
}

std::atomic<bool> g_lds_o[8][16];

template <int LOG2N>
hipError_t launch_onset_t(const PvOnsetParams &p, int groups, hipStream_t st)
{
    using C = SC<LOG2N>;
    const hipError_t e = pv_set_dynamic_lds_once(g_lds_o[LOG2N - 8], (const void *)pv_onset_strength_kernel<LOG2N>, (int)C::LDS_A);
    if (e != hipSuccess) return e;
    const int chains = (p.nframes + p.F - 1) / p.F;
    hipLaunchKernelGGL((pv_onset_strength_kernel<LOG2N>), dim3((unsigned)chains, (unsigned)groups), dim3(TPB), C::LDS_A, st, p);
    return hipGetLastError();
}

}  // namespace

hipError_t pv_launch_onset_strength(int log2n, const float *in, long in_stride, int nch, int G, int nframes, int ha, int F, const double2 *tw64,
                                    const float *hann, int *counts, long count_stride, hipStream_t st)
{
    if (G < 1 || nch % G != 0 || F < 1 || nframes < 1) return hipErrorInvalidValue;
    const PvOnsetParams p{in, in_stride, counts, count_stride, nframes, G, ha, F, tw64, hann};
    return for_log2n(log2n, hipErrorInvalidValue, [&](auto L) { return launch_onset_t<L()>(p, nch / G, st); });
}
