// pv_residue.h -- the above-Nyquist residue, once: what fft.js's in-place real radix-4 DIT leaves at positions N/2+1 .. N-1 of its buffer,
// which the last region of an f < 1 frame reads (pv:133).  The reference's stage structure (bundle:306-442) is re-run on the upper half only: radix-4 base
// blocks when log2 N is even (bundle:468-508), radix-2 when it is odd (bundle:447-463), then the radix-4 stages with their predicated stores (bundle:329-441).
//
// The register kernels rebuild one QUARTER of the buffer at a time (quarter 2 = sub-FFT of xw[4n+2], positions N/2 .. 3N/4; quarter 3 = xw[4n+3]) in a quarter
// buffer Q and add its sources into Y: residue_quarters below, driven by a small struct that a kernel defines next to its own code (what it must supply is listed
// at residue_quarters).  It serves the two reference-width (fp64) copies, residue_scatter_1024_d and residue_scatter_wg16_d; the fp32 copies and pv_chain_kernel's
// residue_upper_half keep their own texts, because their bits or their callers' registers move with this one (DESIGN.md section 3 has the figures).
#pragma once
#include "pv_device_common.h"

namespace {

// radix-4 base block lb of a buffer (bundle:468-508) from its four windowed samples off + q N/4, q = 0..3 (off = base-4 digit reversal of the block)
template <typename V2, typename S>
__device__ __forceinline__ void residue_base4(V2 *Q, int lb, S a, S b, S c, S d)
{
    const S t0 = a + c, t1 = a - c, t2 = b + d, t3 = b - d;
    Q[4 * lb] = V2{t0 + t2, (S)0};
    Q[4 * lb + 1] = V2{t1, -t3};
    Q[4 * lb + 2] = V2{t0 - t2, (S)0};
    Q[4 * lb + 3] = V2{t1, t3};
}
// radix-2 base block lb (bundle:447-463) from the windowed samples off, off + N/2
template <typename V2, typename S>
__device__ __forceinline__ void residue_base2(V2 *Q, int lb, S a, S b)
{
    Q[2 * lb] = V2{a + b, (S)0};
    Q[2 * lb + 1] = V2{a - b, (S)0};
}

// Work item u of a stage with blocks of 2^log2m elements -> (block, butterfly index): a block has the butterflies i = 0 .. hq = 2^log2m / 8, the items
// [0, nblocks * hq) are the butterflies i < hq block by block, the last nblocks items the butterflies i = hq.  (hq is a power of two: a shift and a mask
// instead of a division by a run-time value -- a stage is 1-2 butterflies per thread and is bound by the instructions around them,
// profiles/r05_wg16_phase_clock.md.)
__device__ __forceinline__ void residue_item(int u, int log2m, int nblocks, int &blk, int &i)
{
    const int hq = (1 << log2m) >> 3;
    if (u < nblocks * hq) { blk = u >> (log2m - 3); i = u & (hq - 1); } else { blk = u - nblocks * hq; i = hq; }
}

// Butterfly i of the block of 4 q elements at Q[o] with the twiddles W^e, W^2e, W^3e, and the reference's predicated stores
template <typename V2>
__device__ __forceinline__ void residue_butterfly(V2 *Q, int o, int q, int i, V2 w1, V2 w2, V2 w3)
{
    const int hq = q >> 1;
    const V2 A = Q[o + i];
    const V2 Bv = cmul(Q[o + q + i], w1);
    const V2 C = cmul(Q[o + 2 * q + i], w2);
    const V2 D = cmul(Q[o + 3 * q + i], w3);
    const V2 T0 = cadd(A, C), T1 = csub(A, C), T2 = cadd(Bv, D), T3 = csub(Bv, D);
    Q[o + i] = cadd(T0, T2);
    Q[o + q + i] = V2{T1.x + T3.y, T1.y - T3.x};                          // T1 - j T3
    if (i == 0) {
        Q[o + 2 * q] = csub(T0, T2);                                      // bundle:400-406
    } else if (i != hq) {                                                 // bundle:409-440
        Q[o + q - i] = V2{T1.x - T3.y, -(T1.y + T3.x)};                   // conj(T1 + j T3)
        Q[o + 2 * q - i] = V2{T0.x - T2.x, -(T0.y - T2.y)};               // conj(T0 - T2)
    }
}

// Route of the above-Nyquist source bin b: all of them are owned by the last peak (pv:133), b -> b + up_delta
template <int H>
__device__ __forceinline__ unsigned residue_route(int b, int upper_end, int up_delta, unsigned up_ridx)
{
    const int tgt = b + up_delta;
    return (b >= H && b < upper_end && tgt >= 0 && tgt < H) ? ((up_ridx << 16) | (unsigned)tgt) : NOROUTE;
}

struct NoResidueMark { __device__ __forceinline__ void operator()(int) const {} };

// The quarter-at-a-time form of the register kernels: rebuild the quarters below upper_end in k.Q(), add their sources into Y.  The kernel's struct K supplies
//   V2, LOG2N, T          the complex type, the frame size, the threads that work on one frame (a wave or the workgroup)
//   UNROLL_STAGES         whether the stage loop is unrolled: the callee's registers are the kernel's (tests/test_kernel_resources.py tells the story)
//   ID0                   claim ids count the source bins from ID0
//   Q()                   the quarter buffer, V2[N / 4]
//   sync()                the barrier between the stages (wave_sync or __syncthreads)
//   sample(base, s)       windowed sample s of the frame as the base stage of the quarter at `base` takes it (the frame's stash of xw[4n + 2], or global x Hann)
//   twiddles(i, q, tws, w1, w2, w3)   W_N^e, W_N^2e, W_N^3e for e = i << tws (i <= q / 2, e <= N / 8)
//   rotate(route, v)      the rotation of one source along its route (pv:155-170)
//   add(rt, ys, id)       the NS = N / (4 T) sources of a thread into Y (claim rounds or plain stores), up to the barrier behind them
// mark(k): phase clock of measurement builds (k = 0 base stage, 1.. stages, 7 sources); nothing by default.
template <typename K, typename MARK = NoResidueMark>
__device__ __forceinline__ void residue_quarters(const K &k, int t, int upper_end, int up_delta, unsigned up_ridx, double *dbg_X, MARK mark = MARK{})
{
    using V2 = typename K::V2;
    constexpr int LOG2N = K::LOG2N, N = 1 << LOG2N, H = N / 2 + 1, QN = N / 4, T = K::T;
    constexpr bool BASE4 = (LOG2N % 2) == 0;
    constexpr int NS = QN / T;
    V2 *Q = k.Q();
    for (int base = N / 2; base < N && base < upper_end; base += QN) {
        if (BASE4) {
            constexpr int nd = (LOG2N - 2) / 2;
#pragma unroll
            for (int i = 0; i < NS / 4; i++) {                             // QN / 4 radix-4 blocks per quarter
                const int lb = t + T * i, off = digitrev4(base / 4 + lb, nd);
                residue_base4(Q, lb, k.sample(base, off), k.sample(base, off + N / 4), k.sample(base, off + N / 2), k.sample(base, off + 3 * N / 4));
            }
        } else {
            constexpr int nd = (LOG2N - 1) / 2;
#pragma unroll
            for (int i = 0; i < NS / 2; i++) {                             // QN / 2 radix-2 blocks per quarter
                const int lb = t + T * i, off = digitrev4(base / 2 + lb, nd);
                residue_base2(Q, lb, k.sample(base, off), k.sample(base, off + N / 2));
            }
        }
        k.sync();
        mark(0);
        constexpr int LOG2BASE = BASE4 ? 2 : 1;
        constexpr int STAGE_UNROLL = K::UNROLL_STAGES ? (LOG2N - 2 - LOG2BASE) / 2 : 1;      // all (LOG2N - 2 - LOG2BASE) / 2 stages, or none
#pragma unroll STAGE_UNROLL
        for (int log2m = LOG2BASE + 2; log2m <= LOG2N - 2; log2m += 2) {  // block sizes 4 * base .. N/4 inside the quarter
            const int q = (1 << log2m) >> 2, hq = q >> 1;
            const int nblocks = QN >> log2m;
            auto item = [&](int u) {                                       // the butterflies of a stage touch disjoint elements: any order
                int blk, i;
                residue_item(u, log2m, nblocks, blk, i);
                V2 w1, w2, w3;
                k.twiddles(i, q, LOG2N - log2m, w1, w2, w3);
                residue_butterfly(Q, blk << log2m, q, i, w1, w2, w3);
            };
            if constexpr (QN / 8 + (QN >> (LOG2BASE + 2)) <= T) {          // the largest stage has QN / 8 + QN / (4 * base) items: at most one per thread
                if (t < nblocks * (hq + 1)) item(t);
            } else {
                for (int u = t; u < nblocks * (hq + 1); u += T) item(u);
            }
            k.sync();
            mark(1 + (log2m - LOG2BASE - 2) / 2);
        }
        if (dbg_X)
            for (int i = t; i < QN; i += T) if (base + i >= H) { dbg_X[2 * (base + i)] = (double)Q[i].x; dbg_X[2 * (base + i) + 1] = (double)Q[i].y; }
        unsigned rt[NS];
        V2 ys[NS];
        int id[NS];
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int b = base + t + T * j;
            rt[j] = residue_route<H>(b, upper_end, up_delta, up_ridx);
            ys[j] = k.rotate(rt[j], Q[t + T * j]);
            id[j] = b - K::ID0;
        }
        k.add(rt, ys, id);
        mark(7);
    }
}

}  // namespace
