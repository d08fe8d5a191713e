// pv_stretch_kernels.hip -- phase-locked time stretch (Laroche-Dolson identity phase locking) for gfx950, N = 256 .. 8192.
//
// Per frame: periodic Hann (f32) -> fp64 forward transform (N/2-point complex FFT in LDS + split) -> f32 squared magnitudes -> findPeaks ->
// regions of influence (shiftPeaks at f = 1) -> fixed-point analysis phase q (u32 turns) -> psi += adv (u32) -> every bin rotated by its peak's
// angle psi[P] - q[P] -> fp32 c2r inverse -> Hann -> overlap-add at the synthesis hop.  The algorithm text is DESIGN.md "Time stretch".
//
// Pass structure (one workgroup per (chain of frames, channel)):
//   pass A  q for every frame of the chain (+ the halo frames of pass B and one frame before them for phi); writes the chain's per-bin sums of adv
//   scan    per (channel, bin): exclusive prefix of the chains' sums on top of the carried psi; u32 adds, exact in any order
//   pass B  the chain again from its carry, `halo` frames early for the overlap-add (their psi is the carry minus their adv sum: exact mod 2^32);
//           locks, inverts, overlap-adds and stores; the last chain of a channel writes the carried state
// Every carried quantity is an integer sum or a per-frame function of the input, so any split of a stream into calls or chains gives the same bits.
// Variable tempo (SCHED): frame m consumes its own hop ha_m >= ha and its window ends at the input consumed so far, S[m + 1]; positions and hops come
// from the host's prefix table (PvStretchParams::pos).  The fixed-hop instances (SCHED = false) compute S[m] = m ha and never read a table.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_stretch_device.h"

namespace {

template <int LOG2N, bool SCHED>
__global__ __launch_bounds__(TPB) void pv_stretch_pass_a(PvStretchParams p)
{
    using C = SC<LOG2N>;
    extern __shared__ __align__(16) unsigned char lds[];
    double2 *A = (double2 *)lds;
    unsigned *phi = (unsigned *)(lds + C::A_BYTES);
    unsigned *sm = (unsigned *)(lds + C::A_BYTES + C::H4);
    unsigned *sh = (unsigned *)(lds + C::A_BYTES + 2 * C::H4);
    const int j = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const long hl = C::N - p.ha;
    const float *st = p.state_in + (long)c * p.state_stride;
    const Src src{st, p.in + (long)c * p.in_stride, hl};
    const Sched<SCHED> sc = sched<SCHED>(p, c);
    const int m0 = j * p.F, m1 = min(m0 + p.F, p.nframes);
    const int b = j == 0 ? 0 : m0 - p.halo;
    if (j == 0) {
        const unsigned *phi_state = (const unsigned *)(st + hl + (C::N - p.hs));
        for (int k = tid; k < C::H; k += TPB) phi[k] = phi_state[k];
    } else {
        forward<LOG2N>(A, src, sc.start(b - 1), p.hann, p.tw64);
        for (int k = tid; k < C::H; k += TPB) phi[k] = phase_q(A[k]);
        __syncthreads();
    }
    for (int k = tid; k < C::H; k += TPB) { sm[k] = 0u; sh[k] = 0u; }
#pragma unroll 1
    for (int m = b; m < m1; m++) {
        forward<LOG2N>(A, src, sc.start(m), p.hann, p.tw64);
        const bool main_frame = m >= m0;
        const int ha = sc.hop(m);
        for (int k = tid; k < C::H; k += TPB) {
            const unsigned q = phase_q(A[k]);
            const unsigned adv = advance<LOG2N>(q, phi[k], k, ha, p.hs);
            phi[k] = q;
            if (main_frame) sm[k] += adv; else sh[k] += adv;
        }
        __syncthreads();
    }
    unsigned *out = p.sums + (size_t)(c * p.nchains + j) * 2 * C::H;
    for (int k = tid; k < C::H; k += TPB) { out[k] = sm[k]; out[C::H + k] = sh[k]; }
}

// one thread per (channel, bin): carry_j = psi + sum_{i<j} main_i - halo_j (into the halo slot), psi_out = psi + sum main
__global__ __launch_bounds__(TPB) void pv_stretch_scan(PvStretchParams p, int N)
{
    const int H = N / 2 + 1;
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)p.nch * H) return;
    const int c = (int)(i / H), k = (int)(i % H);
    const long off = (long)(N - p.ha) + (N - p.hs) + H;
    unsigned psi = ((const unsigned *)(p.state_in + (long)c * p.state_stride + off))[k];
    for (int j = 0; j < p.nchains; j++) {
        unsigned *s = p.sums + (size_t)(c * p.nchains + j) * 2 * H;
        const unsigned main_sum = s[k];
        s[H + k] = psi - s[H + k];
        psi += main_sum;
    }
    ((unsigned *)(p.state_out + (long)c * p.state_stride + off))[k] = psi;
}

template <int LOG2N, bool SCHED>
__global__ __launch_bounds__(TPB) void pv_stretch_pass_b(PvStretchParams p)
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
    const int j = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const long hl = N - p.ha;
    const float *st = p.state_in + (long)c * p.state_stride;
    const Src src{st, p.in + (long)c * p.in_stride, hl};
    const Sched<SCHED> sc = sched<SCHED>(p, c);
    const int m0 = j * p.F, m1 = min(m0 + p.F, p.nframes);
    const int b = j == 0 ? 0 : m0 - p.halo;
    const unsigned *carry = p.sums + (size_t)(c * p.nchains + j) * 2 * H + H;
    for (int k = tid; k < H; k += TPB) psi[k] = carry[k];
    if (j == 0) {
        const float *acc = st + hl;
        const unsigned *phi_state = (const unsigned *)(acc + (N - p.hs));
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
        // magnitudes (computeMagnitudes: re^2 + im^2 in fp64, stored as f32), analysis phase, phase advance
        const int ha = sc.hop(m);
        for (int k = tid; k < H; k += TPB) {
            const double2 X = A[k];
            mag[k] = (float)__dadd_rn(__dmul_rn(X.x, X.x), __dmul_rn(X.y, X.y));
            const unsigned q = phase_q(X);
            psi[k] += advance<LOG2N>(q, phi[k], k, ha, p.hs);
            phi[k] = q;
        }
        __syncthreads();
#include "pv_stretch_regions.inc"
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
        for (long i = tid; i < hl; i += TPB) so[i] = src.at(e + i);
        for (int i = tid; i < N - p.hs; i += TPB) so[hl + i] = ring[(base + i) & (N - 1)];
        unsigned *sphi = (unsigned *)(so + hl + (N - p.hs));
        for (int k = tid; k < H; k += TPB) sphi[k] = phi[k];
    }
}

std::atomic<bool> g_lds_a[2][8][16], g_lds_b[2][8][16];

template <int LOG2N, bool SCHED>
hipError_t launch_t(const PvStretchParams &p, hipStream_t st)
{
    using C = SC<LOG2N>;
    hipError_t e = pv_set_dynamic_lds_once(g_lds_a[SCHED][LOG2N - 8], (const void *)pv_stretch_pass_a<LOG2N, SCHED>, (int)C::LDS_A);
    if (e != hipSuccess) return e;
    e = pv_set_dynamic_lds_once(g_lds_b[SCHED][LOG2N - 8], (const void *)pv_stretch_pass_b<LOG2N, SCHED>, (int)C::LDS_B);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)p.nchains, (unsigned)p.nch);
    hipLaunchKernelGGL((pv_stretch_pass_a<LOG2N, SCHED>), grid, dim3(TPB), C::LDS_A, st, p);
    const long scan_threads = (long)p.nch * C::H;
    hipLaunchKernelGGL(pv_stretch_scan, dim3((unsigned)((scan_threads + TPB - 1) / TPB)), dim3(TPB), 0, st, p, C::N);
    hipLaunchKernelGGL((pv_stretch_pass_b<LOG2N, SCHED>), grid, dim3(TPB), C::LDS_B, st, p);
    return hipGetLastError();
}

template <int LOG2N>
hipError_t launch_t(const PvStretchParams &p, hipStream_t st)
{
    return p.pos ? launch_t<LOG2N, true>(p, st) : launch_t<LOG2N, false>(p, st);
}

}  // namespace

bool pv_stretch_supported(int log2n) { return log2n >= 8 && log2n <= 13; }
int pv_stretch_threads() { return TPB; }

size_t pv_stretch_lds_bytes(int log2n, bool pass_b)
{
    switch (log2n) {
#define PV_CASE(L) case L: return pass_b ? SC<L>::LDS_B : SC<L>::LDS_A;
    PV_CASE(8) PV_CASE(9) PV_CASE(10) PV_CASE(11) PV_CASE(12) PV_CASE(13)
#undef PV_CASE
    default: return 0;
    }
}

hipError_t pv_launch_stretch_scan(int log2n, const PvStretchParams &p, hipStream_t st)
{
    if (!pv_stretch_supported(log2n)) return hipErrorInvalidValue;
    const int N = 1 << log2n;
    const long scan_threads = (long)p.nch * (N / 2 + 1);
    hipLaunchKernelGGL(pv_stretch_scan, dim3((unsigned)((scan_threads + TPB - 1) / TPB)), dim3(TPB), 0, st, p, N);
    return hipGetLastError();
}

hipError_t pv_launch_stretch(int log2n, const PvStretchParams &p, hipStream_t st)
{
    switch (log2n) {
    case 8: return launch_t<8>(p, st);
    case 9: return launch_t<9>(p, st);
    case 10: return launch_t<10>(p, st);
    case 11: return launch_t<11>(p, st);
    case 12: return launch_t<12>(p, st);
    case 13: return launch_t<13>(p, st);
    default: return hipErrorInvalidValue;
    }
}
