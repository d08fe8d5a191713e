// pv_choir_kernels.hip -- full-grain harmony voices on the overlap-add path for gfx950: every output sample gathers, voice by voice, the Hann grains of
// that voice that cover it, each read forwards or backwards at a step of its own, divides the voice's own num by its own den and adds the quotient times
// the voice's gain (contract, arithmetic and summation order: pv_choir.h).
//
// The structure is the overlap-add kernels': one workgroup per (tile of PV_TSM_TILE consecutive outputs, channel) stages input samples, the prototype
// table P and the window table Hn in LDS; then every thread runs PV_TSM_R outputs, PV_TSM_THREADS apart, so that the 64 lanes of a wave always work on 64
// consecutive outputs.  The device arithmetic of the sibling files is restated here operation for operation (their resource figures are pinned, so they
// stay as they are).  The staged input is the hull of the voices' source ranges, staged once for all of them, and per output the voices run in order,
// each over its own range of the concatenated grain table.  A grain record, a voice's range and its gain are the same for every lane (uniform indices:
// scalar loads); a voice muted on the workgroup's channel is skipped as a whole.
// The direction bit m and the step s are read with the record, so the four-way choice among the kinds of grain is a branch every lane takes the same way,
// not a divergence:
//   s == 256   the direction selects the span index of the lane's output, e0 = n - D - src0 or e0 = D - n - src0; the sample itself for phi == 0, else 64
//              taps upwards from e0 - 32 whose weights are broadcast reads of P, in both directions.
//   s != 256   the direction selects v and the whole part it is added to: v = 256 (tf - phi) + s u on t - D, or v = -256 (tf + phi) - s u on D - t.
//              Nothing after (the span index of the position, r = v mod 65536) knows the direction.  r differs from lane to lane, so each lane forms its own
//              weights: per tap two LDS gathers of P, one interpolation and one gather of the span.  (q, rem) = (d div den, d mod den) is formed
//              incrementally: a tap moves d by 65536, so the pair moves by (65536 div den, 65536 mod den) with a carry, downwards to the tap under the
//              position and upwards from the one after it; two integer divisions per (output, grain) start the two runs.  The taps that are 0 for every
//              lane are skipped: 2 ceil(max(256, s) / 8) taps run, 64 .. 128.  A zero weight is selected away, never multiplied.
// LDS banks: under a mirrored warped grain the lanes walk the span downwards at stride s / 256; a group of 32 lanes reads the set of words that 32 lanes
// walking upwards at that stride would read, so the conflicts are the forward warped grain's (two-way at worst, at s = 512), and the P gathers depend on r
// only, whose set over a group is again that of a forward grain with another origin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "../pv_mul_rounded.h"
#include "pv_choir.h"

namespace {

__device__ __forceinline__ int lds_word(int e) { return e + (e >> 6); }

// pv_vari.h's weight at table position q with remainder rem (0 from q = 32 Q on: P[32 Q] = P[32 Q + 1] = 0)
__device__ __forceinline__ float warped_weight(const float *P, unsigned q, unsigned rem, float inv_den)
{
    const int qc = (int)min(q, (unsigned)(PV_VARI_HALF * PV_VARI_Q));
    const float p0 = P[qc], p1 = P[qc + 1];
    return fmaf((float)rem * inv_den, p1 - p0, p0);
}

__global__ __launch_bounds__(PV_TSM_THREADS) void pv_choir_kernel(PvChoirParams p)
{
    extern __shared__ float4 lds4[];
    float *xs = (float *)lds4;
    float *P = xs + pv_tsm_span_words(p.span);
    float *Hn = P + PV_VARI_TABLE_WORDS;
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int first = (int)blockIdx.x * PV_TSM_TILE;             // the tile's first output, relative to the call
    const int cnt = min(PV_TSM_TILE, p.nout - first);
    const int j0 = p.out_first + first;                          // its buffer position
    const int2 tl = p.tiles[blockIdx.x];                         // {src0, src_count}, the hull: the same for every lane
    const int src0 = tl.x;                                       // buffer position of span sample e = 0
    const int sc = min(max(tl.y, 0), p.span);                    // staged samples

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
    const int nv = min(max(p.nvoices, 1), PV_CHOIR_MAX_VOICES);
    const int2 *__restrict__ ranges = p.ranges + (size_t)blockIdx.x * (size_t)nv;
    const float *__restrict__ gains = p.gains + ch;
    float *out = p.out + (long)ch * p.out_stride + first;
    for (int k = 0; k < PV_TSM_R; k++) {
        const int nrel = min(tid + k * PV_TSM_THREADS, cnt - 1);         // a thread past the tile's end repeats its last output and stores nothing
        const int n = j0 + nrel;
        float acc = 0.0f;
        for (int v = 0; v < nv; v++) {
            const float gain = gains[v * p.nch];                         // the same for every lane
            if (gain == 0.0f) continue;                                  // muted on this channel: the voice touches nothing
            const int2 rg = ranges[v];                                   // {g_first, g_end}: the same for every lane
            float num = 0.0f, den = 0.0f;
            bool covered = false;
            for (int g = rg.x; g < rg.y; g++) {
                const int4 G = grains[g];                                // {t, w, D, L}: the same for every lane
                const int L = min(max(G.w, 2), PV_TSM_MAX_PERIOD);
                const int dn = min(max(n - G.x, -(1 << 20)), 1 << 20);   // inside +-(tile + max_period + 1) for a range the host made
                const int tf = G.y & (PV_TSM_Q - 1);
                const int u = PV_TSM_Q * dn - tf;
                const int ua = abs(u);
                if (ua >= PV_TSM_Q * L) continue;
                const unsigned u4 = 4u * (unsigned)ua;                   // < 2^22
                const unsigned q = u4 / (unsigned)L, rem = u4 - q * (unsigned)L;
                const int qc = (int)min(q, 1024u);
                const float h0 = Hn[qc], h1 = Hn[qc + 1];
                const float h = fmaf((float)rem * (1.0f / (float)L), h1 - h0, h0);
                if (h == 0.0f) continue;
                const int phi = (G.y >> 8) & (PV_TSM_Q - 1);
                const bool mir = (G.y & PV_CHOIR_MIRROR_BIT) != 0;                                             // uniform
                const int s = min(max(pv_choir_step(G.y), PV_CHOIR_MIN_STEP), PV_CHOIR_MAX_STEP);              // uniform
                float xt;
                if (s == PV_TSM_Q) {                                     // uniform: the far grain, in either direction
                    // the span index of the position n - D (forward) or D - n (mirrored): in [33, src_count - 32) for a grain that covers n, since the
                    // host took it into the tile's hull; formed in unsigned arithmetic, since n - D and D - n alone may pass 2^31, and clamped like every
                    // LDS index
                    const unsigned up = (unsigned)n - (unsigned)G.z, down = (unsigned)G.z - (unsigned)n;
                    const int e0 = (int)((mir ? down : up) - (unsigned)src0);
                    if (phi == 0) {                                      // uniform
                        xt = xs[lds_word(max(min(e0, sc - 1), 0))];
                    } else {
                        const int theta = PV_TSM_Q - phi;
                        const int eb = max(min(e0 - PV_TSM_TAPS / 2, sc - PV_TSM_TAPS), 0);
                        float a = 0.0f, sum = 0.0f;
#pragma unroll 8
                        for (int i = 0; i < PV_TSM_TAPS; i++) {
                            const float w = P[abs(PV_TSM_Q * (i - (PV_TSM_TAPS / 2 - 1)) - theta)]; // at most 32 Q - 1: inside the table
                            a = fmaf(w, xs[lds_word(eb + i)], a);
                            sum += w;
                        }
                        xt = a / sum;
                    }
                } else {                                                 // a warped grain: every lane has its own fraction r
                    const int dw = max(PV_TSM_Q, s), W = s < PV_TSM_Q ? PV_TSM_TAPS / 2 : PV_CHOIR_TAPS / 2;    // uniform
                    const int K = (dw + 7) / 8 - 1;                      // the taps -K .. K + 1 about the position can be non-zero
                    const float inv_den = 1.0f / (float)dw;
                    const unsigned dq = 65536u / (unsigned)dw, dr = 65536u - dq * (unsigned)dw;
                    const int su = s * u;                                // |s u| < 2^29: u is a covered output's
                    const int vv = mir ? -PV_TSM_Q * (tf + phi) - su : PV_TSM_Q * (tf - phi) + su;
                    const unsigned r = (unsigned)vv & 65535u;
                    // the span index of tap 0, m - W + 1 - src0 with m = (t - D) + floor(v / 65536) forward and (D - t) + floor(v / 65536) mirrored, in
                    // wrapping unsigned arithmetic; clamped so that all 2 W taps stay inside the staged count (the launch stages at least 2 PV_CHOIR_TAPS)
                    const unsigned whole = mir ? (unsigned)G.z - (unsigned)G.x : (unsigned)G.x - (unsigned)G.z;
                    const int em = (int)(whole + (unsigned)(vv >> 16) - (unsigned)src0);
                    const int eb = max(min(em - W + 1, sc - 2 * W), 0) + (W - 1 - K);               // tap i = W - 1 - K
                    float a = 0.0f, sum = 0.0f;
                    // taps -K .. 0: d = K 65536 + r downwards to r
                    unsigned d = (unsigned)K * 65536u + r;
                    unsigned qq = d / (unsigned)dw, rr = d - qq * (unsigned)dw;
                    for (int i = 0; i <= K; i++) {
                        const float w = warped_weight(P, qq, rr, inv_den);
                        const float x = xs[lds_word(eb + i)];
                        a = w != 0.0f ? fmaf(w, x, a) : a;
                        sum += w;
                        if (rr < dr) { rr += (unsigned)dw; qq -= 1u; }   // (wraps below 0 after the last tap only: recomputed next)
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
            if (covered) acc = acc + mul_rounded(gain, num / den);       // two roundings: the product on its own, then the add
        }
        if (tid + k * PV_TSM_THREADS < cnt) out[nrel] = acc;
    }
}

std::atomic<bool> g_lds_choir[16];

}  // namespace

hipError_t pv_launch_choir(const PvChoirParams &p, hipStream_t stream)
{
    if (p.nout <= 0 || p.nch <= 0) return hipSuccess;
    if (p.span < 2 * PV_CHOIR_TAPS || pv_tsm_lds_bytes(p.span) > PV_TSM_LDS_BYTES || p.nch > 65535 || p.in_count < 0 || p.nvoices < 1
        || p.nvoices > PV_CHOIR_MAX_VOICES)
        return hipErrorInvalidValue;
    const hipError_t e = pv_set_dynamic_lds_once(g_lds_choir, (const void *)pv_choir_kernel, PV_TSM_LDS_BYTES);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((p.nout + PV_TSM_TILE - 1) / PV_TSM_TILE), (unsigned)p.nch);
    hipLaunchKernelGGL(pv_choir_kernel, grid, dim3(PV_TSM_THREADS), pv_tsm_lds_bytes(p.span), stream, p);
    return hipGetLastError();
}
