// pv_stretch_device.h -- device building blocks of the time-stretch kernels (internal), shared by pv_stretch_kernels.hip (pass A, the scans, pass B)
// and pv_onset_kernels.hip (onset strength), and the log2n dispatch of their launchers.
//
// The two big per-frame blocks of pass B -- findPeaks + the region walk, and the locking + inverse + overlap-add -- are plain code in the one frame
// loop of pv_stretch_pass_b, not functions here: as force-inlined functions they changed the register allocation and instruction selection.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "pv_stretch.h"

namespace {

constexpr int TPB = 256;
constexpr int NOPEAK = 0x7fffffff;

// f(std::integral_constant<int, LOG2N>) for a supported size, `none` for any other: the one place that turns a run-time log2n into a template argument
template <class R, class F>
R for_log2n(int log2n, R none, F f)
{
    switch (log2n) {
#define PV_CASE(L) case L: return f(std::integral_constant<int, L>{});
    PV_CASE(8) PV_CASE(9) PV_CASE(10) PV_CASE(11) PV_CASE(12) PV_CASE(13)
#undef PV_CASE
    default: return none;
    }
}

template <int LOG2N>
struct SC {
    static constexpr int N = 1 << LOG2N, M = N / 2, H = M + 1, LOGM = LOG2N - 1;
    static constexpr int BINS = (H + TPB - 1) / TPB;              // bins per thread (strided loops, and the contiguous segments of the region walk)
    static constexpr int PAIRS = (M / 2 + 1 + TPB - 1) / TPB;     // c2r pairs (k, M - k), k = 0 .. M/2, per thread
    static constexpr size_t A_BYTES = ((size_t)(M + 1) * 16 + 15) / 16 * 16;
    static constexpr size_t H4 = ((size_t)H * 4 + 15) / 16 * 16;
    static constexpr size_t LDS_A = A_BYTES + 3 * H4;                                      // A | phi | sum main | sum halo
    static constexpr size_t LDS_B = A_BYTES + 3 * H4 + (size_t)N * 4 + 2 * TPB * 4;        // A | mag / P | phi | psi | ring[N] | scan[2][TPB]
};

// Sample s of the stream "carried history (N - ha) ++ this call's input"; frame m's window is stream[m ha, m ha + N) (SCHED: Sched::start).
struct Src {
    const float *hist;
    const float *in;
    long hl;
    __device__ __forceinline__ float at(long s) const { return s < hl ? hist[s] : in[s - hl]; }
};

// Sample s of the mix of the G channels starting at a group's first slot: the carried hist (slot stride hist_stride) ++ the input (channel stride
// in_stride).  One f32 rounding per add, in slot order.  The loads go out MIX_BATCH at a time before their adds: a load-add chain would wait one
// memory latency per channel.
constexpr int MIX_BATCH = 4;

struct MixSrc {
    const float *hist;
    const float *in;
    long hl, hist_stride, in_stride;
    int G;
    __device__ __forceinline__ float at(long s) const
    {
        const float *x = s < hl ? hist + s : in + (s - hl);
        const long stride = s < hl ? hist_stride : in_stride;
        float u = 0.0f;
        for (int i0 = 0; i0 < G; i0 += MIX_BATCH) {
            float v[MIX_BATCH];
#pragma unroll
            for (int i = 0; i < MIX_BATCH; i++) v[i] = i0 + i < G ? x[(i0 + i) * stride] : 0.0f;
#pragma unroll
            for (int i = 0; i < MIX_BATCH; i++)
                if (i0 + i < G) u = i0 + i == 0 ? v[0] : __fadd_rn(u, v[i]);
        }
        return u;
    }
};

template <bool LINK>
struct GroupSrc { using type = Src; };
template <>
struct GroupSrc<true> { using type = MixSrc; };

// the source the phase path of a group reads: the slot's own stream, or the mix of the group's G slots starting at slot c0
template <bool LINK>
__device__ __forceinline__ typename GroupSrc<LINK>::type group_src(const PvStretchParams &p, int c0, int G, long hl)
{
    const float *sg = p.state_in + (long)c0 * p.state_stride;
    if constexpr (LINK) return MixSrc{sg, p.in + (long)c0 * p.in_stride, hl, p.state_stride, p.in_stride, G};
    else return Src{sg, p.in + (long)c0 * p.in_stride, hl};
}

// Where frames sit in the stream.  end(n) = S[n], the input consumed by frames 0 .. n-1; frame m's window starts at S[m + 1] - ha (the newest N samples
// once its hop is in: hist is N - ha long) and its hop is S[m + 1] - S[m].  Wave-uniform: the table reads are scalar loads.
template <bool SCHED>
struct Sched {
    const long long *S;       // this channel's row (SCHED only)
    int ha;
    __device__ __forceinline__ long end(int n) const { return SCHED ? (long)S[n] : (long)n * ha; }
    __device__ __forceinline__ long start(int m) const { return SCHED ? (long)S[m + 1] - ha : (long)m * ha; }
    __device__ __forceinline__ int hop(int m) const { return SCHED ? (int)(S[m + 1] - S[m]) : ha; }
};

template <bool SCHED>
__device__ __forceinline__ Sched<SCHED> sched(const PvStretchParams &p, int c)
{
    return Sched<SCHED>{SCHED ? p.pos + (long)c * p.pos_stride : nullptr, p.ha};
}

// X[0 .. M] (double2) of the Hann-windowed frame starting at stream sample s0 of `src` (anything with float at(long)).  Radix-2 DIT on z[n] = x[2n] + j x[2n+1], then the real split.
template <int LOG2N, class S>
__device__ void forward(double2 *A, const S &src, long s0, const float *__restrict__ hann, const double2 *__restrict__ tw)
{
    using C = SC<LOG2N>;
    const int tid = threadIdx.x;
    for (int n = tid; n < C::M; n += TPB) {
        const float x0 = __fmul_rn(src.at(s0 + 2 * n), hann[2 * n]);
        const float x1 = __fmul_rn(src.at(s0 + 2 * n + 1), hann[2 * n + 1]);
        A[__brev((unsigned)n) >> (32 - C::LOGM)] = double2{(double)x0, (double)x1};
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s < C::M; s <<= 1) {
        const int tws = C::N / (2 * s);
        for (int j = tid; j < C::M / 2; j += TPB) {
            const int pos = j & (s - 1);
            const int i0 = ((j - pos) << 1) + pos, i1 = i0 + s;
            const double2 w = tw[pos * tws];
            const double2 a = A[i0], b0 = A[i1];
            const double2 b{b0.x * w.x - b0.y * w.y, b0.x * w.y + b0.y * w.x};
            A[i0] = double2{a.x + b.x, a.y + b.y};
            A[i1] = double2{a.x - b.x, a.y - b.y};
        }
        __syncthreads();
    }
    // X[k] = E + W^k O, X[M - k] = conj(E - W^k O), E = (Z[k] + conj Z[M-k]) / 2, O = (Z[k] - conj Z[M-k]) / 2j
    for (int k = tid; k <= C::M / 2; k += TPB) {
        if (k == 0) {
            const double2 z = A[0];
            A[0] = double2{z.x + z.y, 0.0};
            A[C::M] = double2{z.x - z.y, 0.0};
        } else {
            const double2 zk = A[k], zc0 = A[C::M - k];
            const double2 E{0.5 * (zk.x + zc0.x), 0.5 * (zk.y - zc0.y)};
            const double2 O{0.5 * (zk.y + zc0.y), -0.5 * (zk.x - zc0.x)};
            const double2 w = tw[k];
            const double2 WO{O.x * w.x - O.y * w.y, O.x * w.y + O.y * w.x};
            A[k] = double2{E.x + WO.x, E.y + WO.y};
            if (k != C::M - k) A[C::M - k] = double2{E.x - WO.x, WO.y - E.y};
        }
    }
    __syncthreads();
}

// q = round-to-nearest-even(atan2(Im, Re) / 2 pi * 2^32) mod 2^32; atan2(0, 0) = 0; a bin that is not finite, or a non-finite angle, gives 0
// (the angle of an infinite bin depends on where a transform's arithmetic meets inf - inf: no two transforms agree on it)
__device__ __forceinline__ unsigned phase_q(double2 X)
{
    if ((X.x == 0.0 && X.y == 0.0) || !isfinite(X.x) || !isfinite(X.y)) return 0u;
    const double a = atan2(X.y, X.x);
    if (!isfinite(a)) return 0u;
    return (unsigned)(long long)rint(a * (2147483648.0 / M_PI));
}

// adv = hs k 2^32/N + floor((2 d hs + ha) / (2 ha)) mod 2^32, d = (int32)(q - phi - ha k 2^32/N).  The floor runs in fp64: |2 d hs + ha| < 2^45 is exact
// there and the correctly rounded quotient stays on the exact quotient's side of every integer (half an ulp < 1 / (2 ha) for hs < 2^20).
template <int LOG2N>
__device__ __forceinline__ unsigned advance(unsigned q, unsigned phi, int k, int ha, int hs)
{
    const unsigned e = (unsigned)(((unsigned long long)ha * (unsigned)k) << (32 - LOG2N));
    const int d = (int)(q - phi - e);
    const double num = 2.0 * (double)d * (double)hs + (double)ha;
    const long long fl = (long long)floor(num / (2.0 * (double)ha));
    return (unsigned)(((unsigned long long)hs * (unsigned)k) << (32 - LOG2N)) + (unsigned)fl;
}

// Y = X e^{j theta}, theta = 2 pi (int32)(psi[p] - phi[p]) / 2^32 (phi already holds this frame's q); p < 0: no peak in the frame, Y = 0
__device__ __forceinline__ float2 rotate(double2 X, int p, const unsigned *psi, const unsigned *phi)
{
    if (p < 0) return float2{0.0f, 0.0f};
    const int s = (int)(psi[p] - phi[p]);
    float sn, cs;
    sincospif((float)s * 0x1p-31f, &sn, &cs);
    const float xr = (float)X.x, xi = (float)X.y;
    return float2{__fsub_rn(__fmul_rn(xr, cs), __fmul_rn(xi, sn)), __fadd_rn(__fmul_rn(xr, sn), __fmul_rn(xi, cs))};
}

}  // namespace
