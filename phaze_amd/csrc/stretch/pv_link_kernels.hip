// pv_link_kernels.hip -- linked channels for the time stretch (pv_link_channels): one phase track per group of G consecutive channel slots.
//
// Per group and frame (DESIGN.md "Linked channels"): the mix u = ((x_0 + x_1) + x_2) + ... (f32, slot order) runs the mono phase path of
// pv_stretch_kernels.hip -- Hann, fp64 forward, magnitudes, findPeaks, regions P, q, psi += adv, phi = q -- and every channel of the group rotates
// its OWN spectrum X_c by the mix's angles psi[P] - q[P], then inverts and overlap-adds into its own accumulator.  So the group keeps one phi / psi,
// every channel's bin k turns by the same angle, and the inter-channel phase and amplitude ratios of the input survive.
//
// Pass structure (as the unlinked kernels, G >= 2; G = 1 runs the unlinked kernels):
//   pass A  one workgroup per (chain, group): q of the mix; writes the group's per-bin advance sums
//   scan    pv_stretch_scan over the groups (state stride G slots: reads and writes the psi of slot g G)
//   pass B  one workgroup per (chain, channel): the mix's forward -> mag / q / advance / peaks / regions, then a second forward of the channel's own
//           window into A (the mix's spectrum is dead once P is built), then the unlinked locking, inverse and overlap-add.  The last chain writes
//           the channel's hist / acc and the GROUP's phi / psi into the channel's slot, so every slot of a group carries the group's phases.
// The group's phases are read from slot g G (pass A, the scan, pass B's first chain); a schedule row is the row of slot g G (the host rejects rows
// that differ within a group).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_stretch_device.h"

namespace {

template <int LOG2N, bool SCHED>
__global__ __launch_bounds__(TPB) void pv_link_pass_a(PvStretchParams p, int G)
{
    using C = SC<LOG2N>;
    extern __shared__ __align__(16) unsigned char lds[];
    double2 *A = (double2 *)lds;
    unsigned *phi = (unsigned *)(lds + C::A_BYTES);
    unsigned *sm = (unsigned *)(lds + C::A_BYTES + C::H4);
    unsigned *sh = (unsigned *)(lds + C::A_BYTES + 2 * C::H4);
    const int j = blockIdx.x, g = blockIdx.y, c0 = g * G, tid = threadIdx.x;
    const long hl = C::N - p.ha;
    const float *sg = p.state_in + (long)c0 * p.state_stride;
    const MixSrc mix{sg, p.in + (long)c0 * p.in_stride, hl, p.state_stride, p.in_stride, G};
    const Sched<SCHED> sc = sched<SCHED>(p, c0);
    const int m0 = j * p.F, m1 = min(m0 + p.F, p.nframes);
    const int b = j == 0 ? 0 : m0 - p.halo;
    if (j == 0) {
        const unsigned *phi_state = (const unsigned *)(sg + hl + (C::N - p.hs));
        for (int k = tid; k < C::H; k += TPB) phi[k] = phi_state[k];
    } else {
        forward<LOG2N>(A, mix, sc.start(b - 1), p.hann, p.tw64);
        for (int k = tid; k < C::H; k += TPB) phi[k] = phase_q(A[k]);
        __syncthreads();
    }
    for (int k = tid; k < C::H; k += TPB) { sm[k] = 0u; sh[k] = 0u; }
#pragma unroll 1
    for (int m = b; m < m1; m++) {
        forward<LOG2N>(A, mix, sc.start(m), p.hann, p.tw64);
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
    unsigned *out = p.sums + (size_t)(g * p.nchains + j) * 2 * C::H;
    for (int k = tid; k < C::H; k += TPB) { out[k] = sm[k]; out[C::H + k] = sh[k]; }
}

template <int LOG2N, bool SCHED>
__global__ __launch_bounds__(TPB) void pv_link_pass_b(PvStretchParams p, int G)
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
    const MixSrc mix{sg, p.in + (long)c0 * p.in_stride, hl, p.state_stride, p.in_stride, G};
    const Sched<SCHED> sc = sched<SCHED>(p, c0);
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
        forward<LOG2N>(A, mix, sc.start(b - 1), p.hann, p.tw64);
        for (int k = tid; k < H; k += TPB) phi[k] = phase_q(A[k]);
        for (int i = tid; i < N; i += TPB) ring[i] = 0.0f;
    }
    __syncthreads();
    int base = 0;
    float *outc = p.out + (long)c * p.out_stride;
    const float inv_n = 1.0f / (float)N;
#pragma unroll 1
    for (int m = b; m < m1; m++) {
        forward<LOG2N>(A, mix, sc.start(m), p.hann, p.tw64);
        // the group's phase path on the mix: magnitudes, analysis phase, phase advance
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
        // the channel's own spectrum, rotated by the mix's angles
        forward<LOG2N>(A, own, sc.start(m), p.hann, p.tw64);
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
        unsigned *spsi = sphi + H;
        for (int k = tid; k < H; k += TPB) { sphi[k] = phi[k]; spsi[k] = psi[k]; }
    }
}

std::atomic<bool> g_lds_a[2][8][16], g_lds_b[2][8][16];

template <int LOG2N, bool SCHED>
hipError_t launch_t(const PvStretchParams &p, int G, hipStream_t st)
{
    using C = SC<LOG2N>;
    hipError_t e = pv_set_dynamic_lds_once(g_lds_a[SCHED][LOG2N - 8], (const void *)pv_link_pass_a<LOG2N, SCHED>, (int)C::LDS_A);
    if (e != hipSuccess) return e;
    e = pv_set_dynamic_lds_once(g_lds_b[SCHED][LOG2N - 8], (const void *)pv_link_pass_b<LOG2N, SCHED>, (int)C::LDS_B);
    if (e != hipSuccess) return e;
    const int groups = p.nch / G;
    hipLaunchKernelGGL((pv_link_pass_a<LOG2N, SCHED>), dim3((unsigned)p.nchains, (unsigned)groups), dim3(TPB), C::LDS_A, st, p, G);
    PvStretchParams ps = p;                                           // the scan over groups: slot g G's psi, the group's sums
    ps.nch = groups;
    ps.state_stride = p.state_stride * G;
    e = pv_launch_stretch_scan(LOG2N, ps, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pv_link_pass_b<LOG2N, SCHED>), dim3((unsigned)p.nchains, (unsigned)p.nch), dim3(TPB), C::LDS_B, st, p, G);
    return hipGetLastError();
}

template <int LOG2N>
hipError_t launch_t(const PvStretchParams &p, int G, hipStream_t st)
{
    return p.pos ? launch_t<LOG2N, true>(p, G, st) : launch_t<LOG2N, false>(p, G, st);
}

}  // namespace

hipError_t pv_launch_link(int log2n, const PvStretchParams &p, int G, hipStream_t st)
{
    if (G < 2 || p.nch % G != 0) return hipErrorInvalidValue;
    switch (log2n) {
    case 8: return launch_t<8>(p, G, st);
    case 9: return launch_t<9>(p, G, st);
    case 10: return launch_t<10>(p, G, st);
    case 11: return launch_t<11>(p, G, st);
    case 12: return launch_t<12>(p, G, st);
    case 13: return launch_t<13>(p, G, st);
    default: return hipErrorInvalidValue;
    }
}
