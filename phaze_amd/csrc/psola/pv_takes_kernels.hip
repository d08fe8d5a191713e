// pv_takes_kernels.hip -- per-take plans on the overlap-add path for gfx950: one launch whose workgroups belong to different takes, each with its own
// input, grain table, length and output range (contract, records and occupancy classes: pv_takes.h; arithmetic and summation order: pv_tsm.h).
//
// The structure is pv_tsm_kernels.hip's, whose device arithmetic is restated here operation for operation (that file's resource figures are pinned, so it
// stays as it is): one workgroup per (tile, channel) stages the tile's source range, the prototype table P and the window table Hn in LDS; then every
// thread runs PV_TSM_R outputs, PV_TSM_THREADS apart.
// What differs is where a workgroup finds its work.  blockIdx.x indexes the launch's order[] of tile ids; the tile record names the take, the first
// output, the count, the grain range in the call's concatenated table and the source range; the take record gives the pointers, the strides and the
// positions.  All three are read at an index that is the same for every lane: scalar loads.  Every index is clamped before it is used.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_takes.h"

namespace {

__device__ __forceinline__ int lds_word(int e) { return e + (e >> 6); }

__global__ __launch_bounds__(PV_TSM_THREADS) void pv_takes_kernel(PvTakesParams p)
{
    extern __shared__ float4 lds4[];
    float *xs = (float *)lds4;
    float *P = xs + pv_tsm_span_words(p.span);
    float *Hn = P + PV_VARI_TABLE_WORDS;
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int slot = min((int)blockIdx.x, p.count - 1);
    const int tile = min(max(p.order[slot], 0), p.ntiles - 1);   // the same for every lane, as everything read through it
    const int4 ta = p.tiles[2 * tile];                           // {take, first, g_first, g_end}
    const int4 tb = p.tiles[2 * tile + 1];                       // {src0, src_count, count, 0}
    const PvTakeRec *__restrict__ rec = p.takes + min(max(ta.x, 0), p.ntakes - 1);
    const float *in = rec->in;
    float *outp = rec->out;
    const long long in_stride = rec->in_stride, out_stride = rec->out_stride;
    const long long in_first = rec->in_first, in_count = max(rec->in_count, 0LL);
    const int first = max(ta.y, 0);                              // the tile's first output, relative to the record's out_first
    const int cnt = min(tb.z, PV_TSM_TILE);
    if (cnt <= 0) return;                                        // (the whole workgroup)
    const int j0 = rec->out_first + first;                       // its buffer position
    const int g_first = min(max(ta.z, 0), p.ngrains), g_end = min(max(ta.w, g_first), p.ngrains);
    const int src0 = tb.x;                                       // buffer position of span sample e = 0
    const int sc = min(max(tb.y, 0), p.span);                    // staged samples

    // ---- stage: e -> buffer position src0 + e; in[.. - in_first] where the input has it, zero elsewhere
    const float *in_c = in + (long long)ch * in_stride;
    const long long rel = in_first - (long long)src0;            // the span index of the input's first sample, any sign
    const int e_in0 = (int)min((long long)sc, max(0LL, rel));
    const int e_in1 = (int)max((long long)e_in0, min((long long)sc, rel + in_count));
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
    float *out = outp + (long long)ch * out_stride + first;
    for (int k = 0; k < PV_TSM_R; k++) {
        const int nrel = min(tid + k * PV_TSM_THREADS, cnt - 1);         // a thread past the tile's end repeats its last output and stores nothing
        const int n = j0 + nrel;
        float num = 0.0f, den = 0.0f;
        bool covered = false;
        for (int g = g_first; g < g_end; g++) {
            const int4 G = grains[g];                                    // {t, w, D, L}: the same for every lane
            const int L = min(max(G.w, 2), PV_TSM_MAX_PERIOD);
            const int dn = min(max(n - G.x, -(1 << 20)), 1 << 20);       // inside +-(tile + max_period + 1) for a range the host made
            const int ua = abs(PV_TSM_Q * dn - (G.y & (PV_TSM_Q - 1)));
            if (ua >= PV_TSM_Q * L) continue;
            const unsigned u4 = 4u * (unsigned)ua;                       // < 2^22
            const unsigned q = u4 / (unsigned)L, rem = u4 - q * (unsigned)L;
            const int qc = (int)min(q, 1024u);
            const float h0 = Hn[qc], h1 = Hn[qc + 1];
            const float h = fmaf((float)rem * (1.0f / (float)L), h1 - h0, h0);
            if (h == 0.0f) continue;
            const int phi = (G.y >> 8) & (PV_TSM_Q - 1);
            // n - D - src0 lies in [33, src_count - 32) for a grain that covers n (the host took it into the tile's range); formed without
            // signed overflow, since n - D alone may pass 2^31, and clamped like every LDS index
            const int e0 = (int)((unsigned)n - (unsigned)G.z - (unsigned)src0);
            float xt;
            if (phi == 0) {                                              // uniform
                xt = xs[lds_word(max(min(e0, sc - 1), 0))];
            } else {
                const int theta = PV_TSM_Q - phi;
                const int eb = max(min(e0 - PV_TSM_TAPS / 2, sc - PV_TSM_TAPS), 0);
                float a = 0.0f, s = 0.0f;
#pragma unroll 8
                for (int i = 0; i < PV_TSM_TAPS; i++) {
                    const float w = P[abs(PV_TSM_Q * (i - (PV_TSM_TAPS / 2 - 1)) - theta)];         // at most 32 Q - 1: inside the table
                    a = fmaf(w, xs[lds_word(eb + i)], a);
                    s += w;
                }
                xt = a / s;
            }
            num = fmaf(h, xt, num);
            den += h;
            covered = true;
        }
        if (tid + k * PV_TSM_THREADS < cnt) out[nrel] = covered ? num / den : 0.0f;
    }
}

std::atomic<bool> g_lds_takes[16];

}  // namespace

hipError_t pv_launch_takes(const PvTakesParams &p, hipStream_t stream)
{
    if (p.count <= 0 || p.nch <= 0) return hipSuccess;
    if (p.span < 2 * PV_TSM_TAPS || pv_tsm_lds_bytes(p.span) > PV_TSM_LDS_BYTES || p.nch > 65535 || p.ntiles <= 0 || p.ntakes <= 0 || p.ngrains < 0)
        return hipErrorInvalidValue;
    const hipError_t e = pv_set_dynamic_lds_once(g_lds_takes, (const void *)pv_takes_kernel, PV_TSM_LDS_BYTES);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)p.count, (unsigned)p.nch);
    hipLaunchKernelGGL(pv_takes_kernel, grid, dim3(PV_TSM_THREADS), pv_tsm_lds_bytes(p.span), stream, p);
    return hipGetLastError();
}
