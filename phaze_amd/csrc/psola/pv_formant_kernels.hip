// pv_formant_kernels.hip -- overlap-add of Hann grains that read the input at a step of their own, for gfx950: every output sample gathers the grains
// that cover it, and a grain reads the input one sample per output sample (pv_tsm's far grain) or, WARPED, s / 256 samples per output sample, which moves
// the grain's spectral envelope by that factor: formant shifting (contract, arithmetic and summation order: pv_formant.h).
//
// The structure is pv_tsm_kernels.hip's, whose device arithmetic is restated here operation for operation (that file's resource figures are pinned, so
// it stays as it is): one workgroup per (tile of PV_TSM_TILE consecutive outputs, channel) stages the tile's source range [src0, src0 + src_count), the
// prototype table P and the window table Hn in LDS; every thread runs PV_TSM_R outputs, PV_TSM_THREADS apart, so that the 64 lanes of a wave always
// work on 64 consecutive outputs.  A grain record is the same for every lane (a uniform index: scalar loads), and the waves a grain does not reach skip
// it as a whole.  A launch's LDS is sized by the longest source range among its tiles (p.span).
// What is new is the step s of a record.  It is read with the record, so `s == 256` is a branch every lane takes the same way, not a divergence.  That
// side is pv_tsm's code: the sample itself for phi == 0, else 64 taps whose weights are broadcast reads of P.  On the warped side the fraction r of the
// read position differs from lane to lane, so each lane forms its own weights: per tap two LDS gathers of P (P[q] and P[q + 1]), one interpolation and one
// gather of the span.  (q, rem) = (d div den, d mod den) is formed incrementally as pv_vari_kernel does: a tap moves d by 65536, so the pair moves by
// (65536 div den, 65536 mod den) with a carry, downwards to the tap under the position and upwards from the one after it; two integer divisions per
// (output, grain) start the two runs.  The taps that are 0 for every lane (pv_formant.h) are skipped: 2 ceil(max(256, s) / 8) taps run, 64 .. 128.
// A zero weight is selected away (w != 0 ? fmaf(w, x, a) : a), never multiplied: the non-finite rule of the contract.
// LDS banks (a one-dword LDS read is served in two groups of 32 lanes; lanes of a group conflict on (word mod 32) unless they read the same word):
//   the span.  Lane l reads sample m0 + floor((r0 + 256 s l) / 65536) + i: the lanes walk the span at stride s / 256, between 1/2 and 2.  Below 1 some
//     neighbours share a word (a broadcast: free) and the rest are consecutive: no conflict.  Above 1 the 32 lanes of a group spread over up to 64
//     consecutive samples, so two lanes 32 samples apart can meet on a bank: two-way at worst (every tap at s = 512), where the forward grain has none.  The
//     padded layout e + (e >> 6) shifts the upper part of such a run by one word when it crosses a multiple of 64; it still serves these reads (it neither
//     adds a conflict to a run of stride <= 2 beyond two-way nor is it needed by them: it is kept because the s == 256 side and the staging share the array).
//   P.  Lane l reads P[q0 + floor((r_l + c) / den)] with r_l = (r0 + 256 s l) mod 65536.  For s <= 256 (den = 256) that is q0 + ((s l + c') mod 256): odd s
//     gives 32 different banks, no conflict; an s with 2^k | s gives 256 / gcd(s, 256) words (at most 32) on 32 / gcd(s, 32) banks, so 2-way at s = 128,
//     4-way at s = 192 and 8-way at worst (s = 136, 144, 160, 200 ..).  For s > 256 the advance (256 s mod 65536) / s per lane is fractional and the words
//     scatter: s = 512 is one word for all lanes, s = 384 two words, s = 320 four; in between a few lanes per bank.  These conflicts are the cost of per-lane
//     weights; tools/bench_stretch.py --formant measures it (DESIGN.md "Formant shifting").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_formant.h"

namespace {

__device__ __forceinline__ int lds_word(int e) { return e + (e >> 6); }

// pv_vari.h's weight at table position q with remainder rem (0 from q = 32 Q on: P[32 Q] = P[32 Q + 1] = 0)
__device__ __forceinline__ float warped_weight(const float *P, unsigned q, unsigned rem, float inv_den)
{
    const int qc = (int)min(q, (unsigned)(PV_VARI_HALF * PV_VARI_Q));
    const float p0 = P[qc], p1 = P[qc + 1];
    return fmaf((float)rem * inv_den, p1 - p0, p0);
}

__global__ __launch_bounds__(PV_TSM_THREADS) void pv_formant_kernel(PvTsmParams p)
{
    extern __shared__ float4 lds4[];
    float *xs = (float *)lds4;
    float *P = xs + pv_tsm_span_words(p.span);
    float *Hn = P + PV_VARI_TABLE_WORDS;
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int first = (int)blockIdx.x * PV_TSM_TILE;             // the tile's first output, relative to the call
    const int cnt = min(PV_TSM_TILE, p.nout - first);
    const int j0 = p.out_first + first;                          // its buffer position
    const int4 tl = p.tiles[blockIdx.x];                         // {g_first, g_end, src0, src_count}: the same for every lane
    const int src0 = tl.z;                                       // buffer position of span sample e = 0
    const int sc = min(max(tl.w, 0), p.span);                    // staged samples

    // ---- stage: e -> buffer position src0 + e; in[.. - in_first] where the input has it, zero elsewhere
    const float *in_c = p.in + (long)ch * p.in_stride;
    const long long rel = p.in_first - (long long)src0;          // the span index of the input's first sample, any sign
    const int e_in0 = (int)min((long long)sc, max(0LL, rel));
    const int e_in1 = (int)max((long long)e_in0, min((long long)sc, rel + p.in_count));
    for (int e = tid; e < e_in0; e += PV_TSM_THREADS) xs[lds_word(e)] = 0.0f;
    for (int e = e_in1 + tid; e < sc; e += PV_TSM_THREADS) xs[lds_word(e)] = 0.0f;
    if (e_in1 > e_in0) {
        const long long g0 = -rel;                               // in_c index of e = 0; 0 <= g0 + e < in_count for e_in0 <= e < e_in1
        const int mis = (int)((((uintptr_t)in_c >> 2) + (uintptr_t)(g0 + e_in0)) & 3);            // in_c + g0 + e_in0 - mis is 16-byte aligned
        const int base = e_in0 - mis;
        const int quads = (e_in1 - base + 3) >> 2;
        for (int q = tid; q < quads; q += PV_TSM_THREADS) {
            const int e = base + 4 * q;
            if (e >= e_in0 && e + 4 <= e_in1) {
                const float4 v = *(const float4 *)(in_c + (g0 + e));
                xs[lds_word(e)] = v.x; xs[lds_word(e + 1)] = v.y; xs[lds_word(e + 2)] = v.z; xs[lds_word(e + 3)] = v.w;
            } else {
                for (int u = 0; u < 4; u++)
                    if (e + u >= e_in0 && e + u < e_in1) xs[lds_word(e + u)] = in_c[g0 + e + u];
            }
        }
    }
    {
        const float4 *g4 = (const float4 *)p.ptable;
        for (int k = tid; k < PV_VARI_TABLE_WORDS / 4; k += PV_TSM_THREADS) ((float4 *)P)[k] = g4[k];
        const float4 *h4 = (const float4 *)p.htable;
        for (int k = tid; k < PV_TSM_WINDOW_WORDS / 4; k += PV_TSM_THREADS) ((float4 *)Hn)[k] = h4[k];
    }
    __syncthreads();

    const int4 *__restrict__ grains = p.grains;
    float *out = p.out + (long)ch * p.out_stride + first;
    for (int k = 0; k < PV_TSM_R; k++) {
        const int nrel = min(tid + k * PV_TSM_THREADS, cnt - 1);         // a thread past the tile's end repeats its last output and stores nothing
        const int n = j0 + nrel;
        float num = 0.0f, den = 0.0f;
        bool covered = false;
        for (int g = tl.x; g < tl.y; g++) {
            const int4 G = grains[g];                                    // {t, w, D, L}: the same for every lane
            const int L = min(max(G.w, 2), PV_TSM_MAX_PERIOD);
            const int dn = min(max(n - G.x, -(1 << 20)), 1 << 20);       // inside +-(tile + max_period + 1) for a range the host made
            const int tf = G.y & (PV_TSM_Q - 1);
            const int u = PV_TSM_Q * dn - tf;
            const int ua = abs(u);
            if (ua >= PV_TSM_Q * L) continue;
            const unsigned u4 = 4u * (unsigned)ua;                       // < 2^22
            const unsigned q = u4 / (unsigned)L, rem = u4 - q * (unsigned)L;
            const int qc = (int)min(q, 1024u);
            const float h0 = Hn[qc], h1 = Hn[qc + 1];
            const float h = fmaf((float)rem * (1.0f / (float)L), h1 - h0, h0);
            if (h == 0.0f) continue;
            const int phi = (G.y >> 8) & (PV_TSM_Q - 1);
            const int s = min(max(pv_formant_step(G.y), PV_FORMANT_MIN_STEP), PV_FORMANT_MAX_STEP);      // uniform
            float xt;
            if (s == PV_TSM_Q) {                                         // uniform: pv_tsm's grain
                // the span index of the position n - D: in [33, src_count - 32) for a grain that covers n, since the host took it into the tile's range;
                // formed in unsigned arithmetic, since n - D alone may pass 2^31, and clamped like every LDS index
                const int e0 = (int)((unsigned)n - (unsigned)G.z - (unsigned)src0);
                if (phi == 0) {                                          // uniform
                    xt = xs[lds_word(max(min(e0, sc - 1), 0))];
                } else {
                    const int theta = PV_TSM_Q - phi;
                    const int eb = max(min(e0 - PV_TSM_TAPS / 2, sc - PV_TSM_TAPS), 0);
                    float a = 0.0f, sum = 0.0f;
#pragma unroll 8
                    for (int i = 0; i < PV_TSM_TAPS; i++) {
                        const float w = P[abs(PV_TSM_Q * (i - (PV_TSM_TAPS / 2 - 1)) - theta)];     // at most 32 Q - 1: inside the table
                        a = fmaf(w, xs[lds_word(eb + i)], a);
                        sum += w;
                    }
                    xt = a / sum;
                }
            } else {                                                     // a warped grain: every lane has its own fraction r
                const int dw = max(PV_TSM_Q, s), W = s < PV_TSM_Q ? PV_TSM_TAPS / 2 : PV_FORMANT_TAPS / 2;       // uniform
                const int K = (dw + 7) / 8 - 1;                          // the taps -K .. K + 1 about the position can be non-zero
                const float inv_den = 1.0f / (float)dw;
                const unsigned dq = 65536u / (unsigned)dw, dr = 65536u - dq * (unsigned)dw;
                const int v = PV_TSM_Q * (tf - phi) + s * u;             // |s u| < 2^29: u is a covered output's
                const unsigned r = (unsigned)v & 65535u;
                // the span index of tap 0, m - W + 1 - src0 with m = (t - D) + floor(v / 65536), in wrapping unsigned arithmetic; clamped so that all
                // 2 W taps stay inside the staged count (the launch stages at least 2 PV_FORMANT_TAPS samples)
                const int em = (int)((unsigned)G.x - (unsigned)G.z + (unsigned)(v >> 16) - (unsigned)src0);
                const int eb = max(min(em - W + 1, sc - 2 * W), 0) + (W - 1 - K);                    // tap i = W - 1 - K
                float a = 0.0f, sum = 0.0f;
                // taps -K .. 0: d = K 65536 + r downwards to r
                unsigned d = (unsigned)K * 65536u + r;
                unsigned qq = d / (unsigned)dw, rr = d - qq * (unsigned)dw;
                for (int i = 0; i <= K; i++) {
                    const float w = warped_weight(P, qq, rr, inv_den);
                    const float x = xs[lds_word(eb + i)];
                    a = w != 0.0f ? fmaf(w, x, a) : a;
                    sum += w;
                    if (rr < dr) { rr += (unsigned)dw; qq -= 1u; }       // (wraps below 0 after the last tap only: recomputed next)
                    rr -= dr;
                    qq -= dq;
                }
                // taps 1 .. K + 1: d = 65536 - r upwards
                d = 65536u - r;
                qq = d / (unsigned)dw;
                rr = d - qq * (unsigned)dw;
                for (int i = K + 1; i <= 2 * K + 1; i++) {
                    const float w = warped_weight(P, qq, rr, inv_den);
                    const float x = xs[lds_word(eb + i)];
                    a = w != 0.0f ? fmaf(w, x, a) : a;
                    sum += w;
                    rr += dr;
                    qq += dq;
                    if (rr >= (unsigned)dw) { rr -= (unsigned)dw; qq += 1u; }
                }
                xt = a / sum;
            }
            num = fmaf(h, xt, num);
            den += h;
            covered = true;
        }
        if (tid + k * PV_TSM_THREADS < cnt) out[nrel] = covered ? num / den : 0.0f;
    }
}

std::atomic<bool> g_lds_formant[16];

}  // namespace

hipError_t pv_launch_formant(const PvTsmParams &p, hipStream_t stream)
{
    if (p.nout <= 0 || p.nch <= 0) return hipSuccess;
    if (p.span < 2 * PV_FORMANT_TAPS || pv_tsm_lds_bytes(p.span) > PV_TSM_LDS_BYTES || p.nch > 65535 || p.in_count < 0) return hipErrorInvalidValue;
    const hipError_t e = pv_set_dynamic_lds_once(g_lds_formant, (const void *)pv_formant_kernel, PV_TSM_LDS_BYTES);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((p.nout + PV_TSM_TILE - 1) / PV_TSM_TILE), (unsigned)p.nch);
    hipLaunchKernelGGL(pv_formant_kernel, grid, dim3(PV_TSM_THREADS), pv_tsm_lds_bytes(p.span), stream, p);
    return hipGetLastError();
}
