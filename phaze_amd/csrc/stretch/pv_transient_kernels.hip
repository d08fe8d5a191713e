// pv_transient_kernels.hip -- phase resets and onset strength for the time stretch (pv_transient_process, pv_onset_strength), gfx950, N = 256 .. 8192.
//
// Phase resets (DESIGN.md "Phase resets"): frame m of a group (a channel slot when unlinked) carries a flag r_m, and the recurrence of
// pv_stretch_kernels.hip becomes psi_m = r_m ? q_m : psi_{m-1} + adv_m in every bin (phi_m = q_m either way).  "Add v" and "set to v" compose
// associatively, (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2), all u32 and exact, so any split into calls or chains still gives the same bits.
// The flags come from the host as int32 prefix counts R[0 .. nframes] beside the position table: r_m = R[m + 1] - R[m], and "a reset in [a, b)" is
// R[b] - R[a] > 0, wave-uniform.
//
// Pass structure (one workgroup per (chain of frames, group); LINK = false: a group is one slot, LINK = true: G >= 2 slots, pv_link_kernels.hip):
//   pass A  q for the chain's own frames [m0, m1) (+ frame m0 - 1 for phi); writes TWO pairs per bin, for [m0, t) and [t, m1), t = max(m0, m1 - halo):
//           the value of each part (q at its last reset plus the advances after it, or the plain sum); the parts' flags are table differences
//   scan    per (group, bin): composes the pairs in order on top of the carried psi; chain j + 1's carry is the value after chain j's first pair.  Every
//           chain but the last holds F >= 4 (halo + 1) frames, so the next chain's halo is exactly [t, m1).  (Subtracting the halo's advance sum from the
//           chain's start value, as the plain kernels do, cannot undo a reset inside the halo.)
//   pass B  the plain pass B from that carry, `halo` frames early, with the reset line
// Always on a schedule (the position table): a fixed-hop call with resets is a schedule of constant hops.
//
// Onset strength: per group and frame, c_m = #{k in [1, H - 1): mag_m[k] > 4 mag_{m-1}[k] and mag_m[k] > 2^-20 max_k mag_m}, mag the f32 Re^2 + Im^2 of
// pass B on the stretch's own front end (forward<>, MixSrc).  Both factors are powers of two: the comparisons are exact functions of mag.  A pure
// function of its buffer: frames at the fixed hop ha, frame m's window ends at (m + 1) ha, zeros before the buffer, frame -1 all zeros, no state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_stretch_device.h"

namespace {

template <bool LINK>
struct GroupSrc { using type = Src; };
template <>
struct GroupSrc<true> { using type = MixSrc; };

// the source the phase path of group g reads: the slot's own stream, or the mix of the group's G slots
template <bool LINK>
__device__ __forceinline__ typename GroupSrc<LINK>::type group_src(const PvStretchParams &p, int c0, int G, long hl)
{
    const float *sg = p.state_in + (long)c0 * p.state_stride;
    if constexpr (LINK) return MixSrc{sg, p.in + (long)c0 * p.in_stride, hl, p.state_stride, p.in_stride, G};
    else return Src{sg, p.in + (long)c0 * p.in_stride, hl};
}

template <int LOG2N, bool LINK>
__global__ __launch_bounds__(TPB) void pv_reset_pass_a(PvStretchParams p, int G, const int *rst, long rst_stride)
{
    using C = SC<LOG2N>;
    extern __shared__ __align__(16) unsigned char lds[];
    double2 *A = (double2 *)lds;
    unsigned *phi = (unsigned *)(lds + C::A_BYTES);
    unsigned *v1 = (unsigned *)(lds + C::A_BYTES + C::H4);
    unsigned *v2 = (unsigned *)(lds + C::A_BYTES + 2 * C::H4);
    const int j = blockIdx.x, g = blockIdx.y, c0 = g * G, tid = threadIdx.x;
    const long hl = C::N - p.ha;
    const auto src = group_src<LINK>(p, c0, G, hl);
    const Sched<true> sc = sched<true>(p, c0);
    const int *R = rst + (long)c0 * rst_stride;
    const int m0 = j * p.F, m1 = min(m0 + p.F, p.nframes);
    const int t = max(m0, m1 - p.halo);
    if (j == 0) {
        const unsigned *phi_state = (const unsigned *)(p.state_in + (long)c0 * p.state_stride + hl + (C::N - p.hs));
        for (int k = tid; k < C::H; k += TPB) phi[k] = phi_state[k];
    } else {
        forward<LOG2N>(A, src, sc.start(m0 - 1), p.hann, p.tw64);
        for (int k = tid; k < C::H; k += TPB) phi[k] = phase_q(A[k]);
        __syncthreads();
    }
    for (int k = tid; k < C::H; k += TPB) { v1[k] = 0u; v2[k] = 0u; }
#pragma unroll 1
    for (int m = m0; m < m1; m++) {
        forward<LOG2N>(A, src, sc.start(m), p.hann, p.tw64);
        unsigned *v = m >= t ? v2 : v1;
        const bool reset = R[m + 1] != R[m];
        const int ha = sc.hop(m);
        for (int k = tid; k < C::H; k += TPB) {
            const unsigned q = phase_q(A[k]);
            v[k] = reset ? q : v[k] + advance<LOG2N>(q, phi[k], k, ha, p.hs);
            phi[k] = q;
        }
        __syncthreads();
    }
    unsigned *out = p.sums + (size_t)(g * p.nchains + j) * 2 * C::H;
    for (int k = tid; k < C::H; k += TPB) { out[k] = v1[k]; out[C::H + k] = v2[k]; }
}

// one thread per (group, bin); p.nch counts groups and p.state_stride / rst_stride step from one group's first slot to the next's.  Chain j's second
// slot is read as its [t, m1) pair and then holds pass B's start carry: psi before frame t of chain j - 1 (the carried psi for chain 0).
__global__ __launch_bounds__(TPB) void pv_reset_scan(PvStretchParams p, int N, const int *rst, long rst_stride)
{
    const int H = N / 2 + 1;
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)p.nch * H) return;
    const int c = (int)(i / H), k = (int)(i % H);
    const long off = (long)(N - p.ha) + (N - p.hs) + H;
    const int *R = rst + (long)c * rst_stride;
    unsigned psi = ((const unsigned *)(p.state_in + (long)c * p.state_stride + off))[k];
    unsigned carry = psi;
    for (int j = 0; j < p.nchains; j++) {
        const int m0 = j * p.F, m1 = min(m0 + p.F, p.nframes);
        const int t = max(m0, m1 - p.halo);
        unsigned *s = p.sums + (size_t)(c * p.nchains + j) * 2 * H;
        const unsigned a = s[k], b = s[H + k];
        s[H + k] = carry;
        carry = R[t] != R[m0] ? a : psi + a;
        psi = R[m1] != R[t] ? b : carry + b;
    }
    ((unsigned *)(p.state_out + (long)c * p.state_stride + off))[k] = psi;
}

template <int LOG2N, bool LINK>
__global__ __launch_bounds__(TPB) void pv_reset_pass_b(PvStretchParams p, int G, const int *rst, long rst_stride)
{
    using C = SC<LOG2N>;
    constexpr int N = C::N, M = C::M, H = C::H;
    extern __shared__ __align__(16) unsigned char lds[];
    double2 *A = (double2 *)lds;
    float2 *B = (float2 *)lds;                                        // the inverse transform reuses A's bytes
    float *mag = (float *)(lds + C::A_BYTES);
    int *P = (int *)(lds + C::A_BYTES);                               // ... and the region map reuses mag's
    unsigned *phi = (unsigned *)(lds + C::A_BYTES + C::H4);
    unsigned *psi = (unsigned *)(lds + C::A_BYTES + 2 * C::H4);
    float *ring = (float *)(lds + C::A_BYTES + 3 * C::H4);
    int *scL = (int *)(ring + N), *scF = scL + TPB;
    const int j = blockIdx.x, c = blockIdx.y, g = c / G, c0 = g * G, tid = threadIdx.x;
    const long hl = N - p.ha;
    const float *st = p.state_in + (long)c * p.state_stride;         // the channel's own slot: hist, acc
    const float *sg = p.state_in + (long)c0 * p.state_stride;        // the group's slot: phi
    const Src own{st, p.in + (long)c * p.in_stride, hl};
    const auto src = group_src<LINK>(p, c0, G, hl);
    const Sched<true> sc = sched<true>(p, c0);
    const int *R = rst + (long)c0 * rst_stride;
    const int m0 = j * p.F, m1 = min(m0 + p.F, p.nframes);
    const int b = j == 0 ? 0 : m0 - p.halo;
    const unsigned *carry = p.sums + (size_t)(g * p.nchains + j) * 2 * H + H;
    for (int k = tid; k < H; k += TPB) psi[k] = carry[k];
    if (j == 0) {
        const float *acc = st + hl;
        const unsigned *phi_state = (const unsigned *)(sg + hl + (N - p.hs));
        for (int k = tid; k < H; k += TPB) phi[k] = phi_state[k];
        for (int i = tid; i < N; i += TPB) ring[i] = i < N - p.hs ? acc[i] : 0.0f;
    } else {
        forward<LOG2N>(A, src, sc.start(b - 1), p.hann, p.tw64);
        for (int k = tid; k < H; k += TPB) phi[k] = phase_q(A[k]);
        for (int i = tid; i < N; i += TPB) ring[i] = 0.0f;
    }
    __syncthreads();
    int base = 0;
    float *outc = p.out + (long)c * p.out_stride;
    const float inv_n = 1.0f / (float)N;
#pragma unroll 1
    for (int m = b; m < m1; m++) {
        forward<LOG2N>(A, src, sc.start(m), p.hann, p.tw64);
        // magnitudes, analysis phase, and the phase advance or the reset psi := q
        const bool reset = R[m + 1] != R[m];
        const int ha = sc.hop(m);
        for (int k = tid; k < H; k += TPB) {
            const double2 X = A[k];
            mag[k] = (float)__dadd_rn(__dmul_rn(X.x, X.x), __dmul_rn(X.y, X.y));
            const unsigned q = phase_q(X);
            psi[k] = reset ? q : psi[k] + advance<LOG2N>(q, phi[k], k, ha, p.hs);
            phi[k] = q;
        }
        __syncthreads();
#include "pv_stretch_regions.inc"
        // linked: the channel's own spectrum, rotated by the mix's angles
        if constexpr (LINK) forward<LOG2N>(A, own, sc.start(m), p.hann, p.tw64);
#include "pv_stretch_synth.inc"
        const bool emit = m >= m0;
        for (int i = tid; i < p.hs; i += TPB) {
            const int r = (base + i) & (N - 1);
            if (emit) outc[(long)m * p.hs + i] = ring[r];
            ring[r] = 0.0f;
        }
        base = (base + p.hs) & (N - 1);
        __syncthreads();
    }
    if (j == p.nchains - 1) {
        float *so = p.state_out + (long)c * p.state_stride;
        const long e = sc.end(p.nframes);
        for (long i = tid; i < hl; i += TPB) so[i] = own.at(e + i);
        for (int i = tid; i < N - p.hs; i += TPB) so[hl + i] = ring[(base + i) & (N - 1)];
        unsigned *sphi = (unsigned *)(so + hl + (N - p.hs));
        for (int k = tid; k < H; k += TPB) sphi[k] = phi[k];
        if constexpr (LINK) {                                         // every slot of a group carries the group's phases (unlinked: the scan wrote psi)
            unsigned *spsi = sphi + H;
            for (int k = tid; k < H; k += TPB) spsi[k] = psi[k];
        }
    }
}

// ---- onset strength ----

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

std::atomic<bool> g_lds_a[2][8][16], g_lds_b[2][8][16], g_lds_o[8][16];

template <int LOG2N, bool LINK>
hipError_t launch_reset_t(const PvStretchParams &p, int G, const int *rst, long rst_stride, hipStream_t st)
{
    using C = SC<LOG2N>;
    hipError_t e = pv_set_dynamic_lds_once(g_lds_a[LINK][LOG2N - 8], (const void *)pv_reset_pass_a<LOG2N, LINK>, (int)C::LDS_A);
    if (e != hipSuccess) return e;
    e = pv_set_dynamic_lds_once(g_lds_b[LINK][LOG2N - 8], (const void *)pv_reset_pass_b<LOG2N, LINK>, (int)C::LDS_B);
    if (e != hipSuccess) return e;
    const int groups = p.nch / G;
    hipLaunchKernelGGL((pv_reset_pass_a<LOG2N, LINK>), dim3((unsigned)p.nchains, (unsigned)groups), dim3(TPB), C::LDS_A, st, p, G, rst, rst_stride);
    PvStretchParams ps = p;                                           // the scan over groups: slot g G's psi and flag row, the group's pairs
    ps.nch = groups;
    ps.state_stride = p.state_stride * G;
    const long scan_threads = (long)groups * C::H;
    hipLaunchKernelGGL(pv_reset_scan, dim3((unsigned)((scan_threads + TPB - 1) / TPB)), dim3(TPB), 0, st, ps, C::N, rst, rst_stride * G);
    hipLaunchKernelGGL((pv_reset_pass_b<LOG2N, LINK>), dim3((unsigned)p.nchains, (unsigned)p.nch), dim3(TPB), C::LDS_B, st, p, G, rst, rst_stride);
    return hipGetLastError();
}

template <int LOG2N>
hipError_t launch_reset_t(const PvStretchParams &p, int G, const int *rst, long rst_stride, hipStream_t st)
{
    return G > 1 ? launch_reset_t<LOG2N, true>(p, G, rst, rst_stride, st) : launch_reset_t<LOG2N, false>(p, 1, rst, rst_stride, st);
}

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

hipError_t pv_launch_stretch_reset(int log2n, const PvStretchParams &p, int G, const int *rst, long rst_stride, hipStream_t st)
{
    if (G < 1 || p.nch % G != 0 || !p.pos || !rst) return hipErrorInvalidValue;
    switch (log2n) {
    case 8: return launch_reset_t<8>(p, G, rst, rst_stride, st);
    case 9: return launch_reset_t<9>(p, G, rst, rst_stride, st);
    case 10: return launch_reset_t<10>(p, G, rst, rst_stride, st);
    case 11: return launch_reset_t<11>(p, G, rst, rst_stride, st);
    case 12: return launch_reset_t<12>(p, G, rst, rst_stride, st);
    case 13: return launch_reset_t<13>(p, G, rst, rst_stride, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t pv_launch_onset_strength(int log2n, const float *in, long in_stride, int nch, int G, int nframes, int ha, int F, const double2 *tw64,
                                    const float *hann, int *counts, long count_stride, hipStream_t st)
{
    if (G < 1 || nch % G != 0 || F < 1 || nframes < 1) return hipErrorInvalidValue;
    const PvOnsetParams p{in, in_stride, counts, count_stride, nframes, G, ha, F, tw64, hann};
    switch (log2n) {
    case 8: return launch_onset_t<8>(p, nch / G, st);
    case 9: return launch_onset_t<9>(p, nch / G, st);
    case 10: return launch_onset_t<10>(p, nch / G, st);
    case 11: return launch_onset_t<11>(p, nch / G, st);
    case 12: return launch_onset_t<12>(p, nch / G, st);
    case 13: return launch_onset_t<13>(p, nch / G, st);
    default: return hipErrorInvalidValue;
    }
}
