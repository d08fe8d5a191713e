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
#include "pv_stretch.h"

namespace {

constexpr int TPB = 256;
constexpr int NOPEAK = 0x7fffffff;

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

// X[0 .. M] (double2) of the Hann-windowed frame starting at stream sample s0.  Radix-2 DIT on z[n] = x[2n] + j x[2n+1], then the real split.
template <int LOG2N>
__device__ void forward(double2 *A, const Src &src, long s0, const float *__restrict__ hann, const double2 *__restrict__ tw)
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
