// pv_stretch_kernels.hip -- phase-locked time stretch (Laroche-Dolson identity phase locking) for gfx950, N = 256 .. 8192: one pass A and one pass B
// template for the fixed hop, variable tempo, linked channels and phase resets.
//
// Per frame: periodic Hann (f32) -> fp64 forward transform (N/2-point complex FFT in LDS + split) -> f32 squared magnitudes -> findPeaks ->
// regions of influence (shiftPeaks at f = 1) -> fixed-point analysis phase q (u32 turns) -> psi += adv (u32) -> every bin rotated by its peak's
// angle psi[P] - q[P] -> fp32 c2r inverse -> Hann -> overlap-add at the synthesis hop.  The algorithm text is DESIGN.md "Time stretch".
//
// Pass structure (a chain is p.F consecutive frames; a group is one channel slot, or with LINK G >= 2 consecutive slots):
//   pass A  one workgroup per (chain, group): q for every frame of the chain (+ the halo frames of pass B and one frame before them for phi); writes the
//           chain's per-bin sums of adv, {main frames, halo frames}
//   scan    per (group, bin): exclusive prefix of the chains' sums on top of the carried psi; u32 adds, exact in any order
//   pass B  one workgroup per (chain, channel): the chain again from its carry, `halo` frames early for the overlap-add (their psi is the carry minus
//           their adv sum: exact mod 2^32); locks, inverts, overlap-adds and stores; the last chain of a channel writes the carried state
// Every carried quantity is an integer sum or a per-frame function of the input, so any split of a stream into calls or chains gives the same bits.
//
// SCHED, variable tempo: frame m consumes its own hop ha_m >= ha and its window ends at the input consumed so far, S[m + 1]; positions and hops come
// from the host's prefix table (PvStretchParams::pos).  The fixed-hop instances compute S[m] = m ha and never read a table.
//
// LINK, linked channels (DESIGN.md "Linked channels"): the mix u = ((x_0 + x_1) + x_2) + ... (f32, slot order) of a group runs the mono phase path --
// Hann, forward, magnitudes, findPeaks, regions P, q, psi, phi -- and every channel of the group rotates its OWN spectrum X_c by the mix's angles
// psi[P] - q[P], then inverts and overlap-adds into its own accumulator: pass B runs a second forward of the channel's own window into A once P is
// built (the mix's spectrum is dead by then).  So the group keeps one phi / psi, every channel's bin k turns by the same angle, and the inter-channel
// phase and amplitude ratios of the input survive.  The group's phases are read from slot g G (pass A, the scan with a state stride of G slots, pass
// B's first chain) and the last chain writes them into every slot of the group; a schedule or flag row is the row of slot g G (the host rejects rows
// that differ within a group).
//
// RESET, phase resets (DESIGN.md "Phase resets"; always on a schedule: a fixed-hop call with resets is a schedule of constant hops): frame m of a group
// carries a flag r_m and the recurrence becomes psi_m = r_m ? q_m : psi_{m-1} + adv_m in every bin (phi_m = q_m either way).  "Add v" and "set to v"
// compose associatively, (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2), all u32 and exact, so any split into calls or chains still gives the
// same bits.  The flags come from the host as int32 prefix counts R[0 .. nframes] beside the position table: r_m = R[m + 1] - R[m], and "a reset in
// [a, b)" is R[b] - R[a] > 0, wave-uniform.  Subtracting the halo's advance sum from the chain's start value, as the plain scan does, cannot undo a
// reset inside the halo, so pass A takes the chain's own frames [m0, m1) only (+ frame m0 - 1 for phi) and writes TWO values per bin, for [m0, t)
// and [t, m1), t = max(m0, m1 - halo): q at the part's last reset plus the advances after it, or the plain sum; the parts' flags are table
// differences.  pv_reset_scan composes them in order on top of the carried psi; chain j + 1's carry is the value after chain j's first part.  Every
// chain but the last holds F >= 4 (halo + 1) frames, so the next chain's halo is exactly [t, m1).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_stretch_device.h"

namespace {

// `group` (G) is read by the LINK instances only, rst and rst_stride by the RESET ones
template <int LOG2N, bool SCHED, bool LINK, bool RESET>
__global__ __launch_bounds__(TPB) void pv_stretch_pass_a(PvStretchParams p, int group, const int *rst, long rst_stride)
{
    static_assert(SCHED || !RESET, "resets run on a schedule");
    using C = SC<LOG2N>;
    extern __shared__ __align__(16) unsigned char lds[];
    double2 *A = (double2 *)lds;
    unsigned *phi = (unsigned *)(lds + C::A_BYTES);
    unsigned *s1 = (unsigned *)(lds + C::A_BYTES + C::H4);           // the main frames' sum; RESET: the value of [m0, t)
    unsigned *s2 = (unsigned *)(lds + C::A_BYTES + 2 * C::H4);       // the halo frames' sum; RESET: the value of [t, m1)
    const int G = LINK ? group : 1;
    const int j = blockIdx.x, g = blockIdx.y, c0 = g * G, tid = threadIdx.x;
    const long hl = C::N - p.ha;
    const auto src = group_src<LINK>(p, c0, G, hl);
    const Sched<SCHED> sc = sched<SCHED>(p, c0);
    const int *R = RESET ? rst + (long)c0 * rst_stride : nullptr;
    const int m0 = j * p.F, m1 = min(m0 + p.F, p.nframes);
    const int b = RESET ? m0 : j == 0 ? 0 : m0 - p.halo;              // the first frame
    const int t = RESET ? max(m0, m1 - p.halo) : m0;                  // RESET: where the second part starts
    if (j == 0) {
        const unsigned *phi_state = (const unsigned *)(p.state_in + (long)c0 * p.state_stride + hl + (C::N - p.hs));
        for (int k = tid; k < C::H; k += TPB) phi[k] = phi_state[k];
    } else {
        forward<LOG2N>(A, src, sc.start(b - 1), p.hann, p.tw64);
        for (int k = tid; k < C::H; k += TPB) phi[k] = phase_q(A[k]);
        __syncthreads();
    }
    for (int k = tid; k < C::H; k += TPB) { s1[k] = 0u; s2[k] = 0u; }
#pragma unroll 1
    for (int m = b; m < m1; m++) {
        forward<LOG2N>(A, src, sc.start(m), p.hann, p.tw64);
        const int ha = sc.hop(m);
        if constexpr (RESET) {
            unsigned *v = m >= t ? s2 : s1;
            const bool reset = R[m + 1] != R[m];
            for (int k = tid; k < C::H; k += TPB) {
                const unsigned q = phase_q(A[k]);
                v[k] = reset ? q : v[k] + advance<LOG2N>(q, phi[k], k, ha, p.hs);
                phi[k] = q;
            }
        } else {
            const bool main_frame = m >= m0;
            for (int k = tid; k < C::H; k += TPB) {
                const unsigned q = phase_q(A[k]);
                const unsigned adv = advance<LOG2N>(q, phi[k], k, ha, p.hs);
                phi[k] = q;
                if (main_frame) s1[k] += adv; else s2[k] += adv;
            }
        }
        __syncthreads();
    }
    unsigned *out = p.sums + (size_t)(g * p.nchains + j) * 2 * C::H;
    for (int k = tid; k < C::H; k += TPB) { out[k] = s1[k]; out[C::H + k] = s2[k]; }
}

// The scans: one thread per (group, bin); p.nch counts groups and p.state_stride (rst_stride) steps from one group's first slot to the next's.
// plain: carry_j = psi + sum_{i<j} main_i - halo_j (into the halo slot), psi_out = psi + sum main
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

// resets: chain j's second slot is read as its [t, m1) part and then holds pass B's start carry: psi before frame t of chain j - 1 (the carried psi
// for chain 0)
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

template <int LOG2N, bool SCHED, bool LINK, bool RESET>
__global__ __launch_bounds__(TPB) void pv_stretch_pass_b(PvStretchParams p, int group, const int *rst, long rst_stride)
{
    static_assert(SCHED || !RESET, "resets run on a schedule");
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
    const int G = LINK ? group : 1;
    const int j = blockIdx.x, c = blockIdx.y, g = c / G, c0 = g * G, tid = threadIdx.x;
    const long hl = N - p.ha;
    const float *st = p.state_in + (long)c * p.state_stride;         // the channel's own slot: hist, acc
    const float *sg = p.state_in + (long)c0 * p.state_stride;        // the group's slot: phi
    const Src own{st, p.in + (long)c * p.in_stride, hl};
    const auto src = group_src<LINK>(p, c0, G, hl);                   // feeds the phase path
    const Sched<SCHED> sc = sched<SCHED>(p, c0);
    const int *R = RESET ? rst + (long)c0 * rst_stride : nullptr;
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
        // magnitudes (computeMagnitudes: re^2 + im^2 in fp64, stored as f32), analysis phase, and the phase advance or the reset psi := q
        bool reset = false;
        if constexpr (RESET) reset = R[m + 1] != R[m];
        const int ha = sc.hop(m);
        for (int k = tid; k < H; k += TPB) {
            const double2 X = A[k];
            mag[k] = (float)__dadd_rn(__dmul_rn(X.x, X.x), __dmul_rn(X.y, X.y));
            const unsigned q = phase_q(X);
            psi[k] = reset ? q : psi[k] + advance<LOG2N>(q, phi[k], k, ha, p.hs);
            phi[k] = q;
        }
        __syncthreads();

        // ---- peaks and regions: findPeaks on mag[0 .. H), then P[k] := the peak whose region of influence holds bin k (shiftPeaks at f = 1), -1 when
        // the frame has no peak.  P aliases mag; scL / scF hold TPB ints each.
        // findPeaks: strict maximum over +-2 bins, k in [2, H - 2)
        unsigned fl = 0;
#pragma unroll
        for (int i = 0; i < C::BINS; i++) {
            const int k = tid + i * TPB;
            if (k >= 2 && k < H - 2) {
                const float v = mag[k];
                const bool pk = !(mag[k - 1] >= v || mag[k - 2] >= v || mag[k + 1] >= v || mag[k + 2] >= v);
                fl |= (pk ? 1u : 0u) << i;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < C::BINS; i++) {
            const int k = tid + i * TPB;
            if (k < H) P[k] = ((fl >> i) & 1u) ? k : NOPEAK;
        }
        __syncthreads();
        // regions: thread t walks the bins [t BINS, (t+1) BINS); the nearest peaks outside its segment come from a prefix max / suffix min over threads
        const int k0 = min(tid * C::BINS, H), k1 = min(k0 + C::BINS, H);
        {
            int lastp = -1, firstp = NOPEAK;
            for (int k = k0; k < k1; k++)
                if (P[k] != NOPEAK) { if (firstp == NOPEAK) firstp = k; lastp = k; }
            scL[tid] = lastp;
            scF[tid] = firstp;
        }
        __syncthreads();
#pragma unroll 1
        for (int off = 1; off < TPB; off <<= 1) {
            const int l = tid >= off ? scL[tid - off] : -1;
            const int f = tid + off < TPB ? scF[tid + off] : NOPEAK;
            __syncthreads();
            scL[tid] = max(scL[tid], l);
            scF[tid] = min(scF[tid], f);
            __syncthreads();
        }
        {
            int prev = tid > 0 ? scL[tid - 1] : -1;
            int next = tid + 1 < TPB ? scF[tid + 1] : NOPEAK;
            for (int k = k1 - 1; k >= k0; k--) {                      // P[k] := smallest peak >= k
                if (P[k] == k) next = k;
                P[k] = next;
            }
            for (int k = k0; k < k1; k++) {                           // region rule: between peaks a < b, bin k goes to b iff b - k <= floor((b - a) / 2)
                const int n = P[k];
                int r;
                if (n == k) { prev = k; r = k; }
                else if (prev < 0) r = n == NOPEAK ? -1 : n;
                else if (n == NOPEAK) r = prev;
                else r = (n - k <= (n - prev) / 2) ? n : prev;
                P[k] = r;
            }
        }
        __syncthreads();

        // linked: the channel's own spectrum, rotated by the mix's angles
        if constexpr (LINK) forward<LOG2N>(A, own, sc.start(m), p.hann, p.tw64);

        // ---- synthesis: every bin A[k] rotated by its peak's angle psi[P] - phi[P] (rotate), the fp32 c2r inverse in B (aliasing A), Hann and
        // overlap-add scaled by hs / N into ring[base ..] (mod N).
        // locking + c2r pre-pass: Z[k] = E + jD, Z[M-k] = conj E + j conj D, E = Y[k] + conj Y[M-k], D = W^-k (Y[k] - conj Y[M-k]) (Im of Y[0], Y[M] dropped)
        float2 zlo[C::PAIRS], zhi[C::PAIRS];
#pragma unroll
        for (int i = 0; i < C::PAIRS; i++) {
            const int k = tid + i * TPB;
            zlo[i] = zhi[i] = float2{0.0f, 0.0f};
            if (k == 0) {
                const float r0 = rotate(A[0], P[0], psi, phi).x, rM = rotate(A[M], P[M], psi, phi).x;
                zlo[i] = float2{r0 + rM, r0 - rM};
            } else if (k <= M / 2) {
                const float2 yk = rotate(A[k], P[k], psi, phi), yc = rotate(A[M - k], P[M - k], psi, phi);
                const float2 E{yk.x + yc.x, yk.y - yc.y};
                const float2 Dm{yk.x - yc.x, yk.y + yc.y};
                const float2 w = p.tw32[k];
                const float2 D{__fadd_rn(__fmul_rn(Dm.x, w.x), __fmul_rn(Dm.y, w.y)), __fsub_rn(__fmul_rn(Dm.y, w.x), __fmul_rn(Dm.x, w.y))};
                zlo[i] = float2{E.x - D.y, E.y + D.x};
                zhi[i] = float2{E.x + D.y, D.x - E.y};
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < C::PAIRS; i++) {
            const int k = tid + i * TPB;
            if (k <= M / 2) {
                B[k] = zlo[i];
                if (k != 0 && k != M - k) B[M - k] = zhi[i];
            }
        }
        __syncthreads();
        // inverse: radix-2 DIF, natural order in, bit-reversed out, fp32
#pragma unroll 1
        for (int s = M / 2; s >= 1; s >>= 1) {
            const int tws = N / (2 * s);
            for (int jj = tid; jj < M / 2; jj += TPB) {
                const int pos = jj & (s - 1);
                const int i0 = ((jj - pos) << 1) + pos, i1 = i0 + s;
                const float2 w = p.tw32[pos * tws];                  // conj(w) = exp(+2 pi j pos / 2s)
                const float2 a = B[i0], bb = B[i1];
                const float2 d{a.x - bb.x, a.y - bb.y};
                B[i0] = float2{a.x + bb.x, a.y + bb.y};
                B[i1] = float2{__fadd_rn(__fmul_rn(d.x, w.x), __fmul_rn(d.y, w.y)), __fsub_rn(__fmul_rn(d.y, w.x), __fmul_rn(d.x, w.y))};
            }
            __syncthreads();
        }
        // frame = Hann * f32(Re IDFT / N); ring += frame * hs / N
        for (int n = tid; n < M; n += TPB) {
            const float2 z = B[__brev((unsigned)n) >> (32 - C::LOGM)];
            const float x0 = __fmul_rn(__fmul_rn(z.x, inv_n), p.hann[2 * n]);
            const float x1 = __fmul_rn(__fmul_rn(z.y, inv_n), p.hann[2 * n + 1]);
            const int r0 = (base + 2 * n) & (N - 1), r1 = (base + 2 * n + 1) & (N - 1);
            ring[r0] = __fadd_rn(ring[r0], __fmul_rn(x0, p.ola_scale));
            ring[r1] = __fadd_rn(ring[r1], __fmul_rn(x1, p.ola_scale));
        }
        __syncthreads();

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
        for (int k = tid; k < H; k += TPB) {
            sphi[k] = phi[k];
            if constexpr (LINK) spsi[k] = psi[k];                     // every slot of a group carries the group's phases (unlinked: the scan wrote psi)
        }
    }
}

std::atomic<bool> g_lds[2][2][2][6][2][16];                           // [SCHED][LINK][RESET][LOG2N - 8][pass A, pass B][device]

template <int LOG2N, bool SCHED, bool LINK, bool RESET>
hipError_t launch_t(const PvStretchParams &p, int G, const int *rst, long rst_stride, hipStream_t st)
{
    using C = SC<LOG2N>;
    const auto pass_a = pv_stretch_pass_a<LOG2N, SCHED, LINK, RESET>, pass_b = pv_stretch_pass_b<LOG2N, SCHED, LINK, RESET>;
    auto &done = g_lds[SCHED][LINK][RESET][LOG2N - 8];
    hipError_t e = pv_set_dynamic_lds_once(done[0], (const void *)pass_a, (int)C::LDS_A);
    if (e != hipSuccess) return e;
    e = pv_set_dynamic_lds_once(done[1], (const void *)pass_b, (int)C::LDS_B);
    if (e != hipSuccess) return e;
    const int groups = p.nch / G;
    hipLaunchKernelGGL(pass_a, dim3((unsigned)p.nchains, (unsigned)groups), dim3(TPB), C::LDS_A, st, p, G, rst, rst_stride);
    PvStretchParams ps = p;                                           // the scan over groups: slot g G's psi and flag row, the group's sums
    ps.nch = groups;
    ps.state_stride = p.state_stride * G;
    const dim3 scan_grid((unsigned)(((long)groups * C::H + TPB - 1) / TPB));
    if constexpr (RESET) hipLaunchKernelGGL(pv_reset_scan, scan_grid, dim3(TPB), 0, st, ps, C::N, rst, rst_stride * G);
    else hipLaunchKernelGGL(pv_stretch_scan, scan_grid, dim3(TPB), 0, st, ps, C::N);
    hipLaunchKernelGGL(pass_b, dim3((unsigned)p.nchains, (unsigned)p.nch), dim3(TPB), C::LDS_B, st, p, G, rst, rst_stride);
    return hipGetLastError();
}

}  // namespace

bool pv_stretch_supported(int log2n) { return log2n >= 8 && log2n <= 13; }
int pv_stretch_threads() { return TPB; }

size_t pv_stretch_lds_bytes(int log2n, bool pass_b)
{
    return for_log2n(log2n, (size_t)0, [&](auto L) -> size_t { return pass_b ? SC<L()>::LDS_B : SC<L()>::LDS_A; });
}

hipError_t pv_launch_stretch(int log2n, const PvStretchParams &p, int G, const int *rst, long rst_stride, hipStream_t st)
{
    if (G < 1 || p.nch % G != 0 || (rst && !p.pos)) return hipErrorInvalidValue;
    return for_log2n(log2n, hipErrorInvalidValue, [&](auto L) {
        constexpr int LOG2N = L();
        if (rst) return G > 1 ? launch_t<LOG2N, true, true, true>(p, G, rst, rst_stride, st) : launch_t<LOG2N, true, false, true>(p, G, rst, rst_stride, st);
        if (p.pos) return G > 1 ? launch_t<LOG2N, true, true, false>(p, G, rst, rst_stride, st) : launch_t<LOG2N, true, false, false>(p, G, rst, rst_stride, st);
        return G > 1 ? launch_t<LOG2N, false, true, false>(p, G, rst, rst_stride, st) : launch_t<LOG2N, false, false, false>(p, G, rst, rst_stride, st);
    });
}
