// pv_psola_kernels.hip -- pitch-synchronous overlap-add for gfx950: every output sample gathers the Hann grains that cover it (contract, arithmetic
// and summation order: pv_psola.h).
//
// One workgroup per (tile of PV_PSOLA_TILE consecutive outputs, channel).  It stages the tile's input span, the prototype table P and the window
// table Hn in LDS; then every thread runs PV_PSOLA_R outputs, PV_PSOLA_THREADS apart, one after the other, so that the 64 lanes of a wave always
// work on 64 consecutive outputs.  Per output the thread walks the tile's grain range, grain index ascending.  A grain record is the same for every
// lane (a uniform index into global memory: scalar loads), so the window test is a compare on a wave-uniform record, the waves a grain does not
// reach skip it as a whole, and the 64 weights of a fractionally shifted grain, which depend on the grain alone, are broadcast reads of P.  Per tap
// a lane reads one input sample from the padded span and does one multiply-add.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_psola.h"

namespace {

__device__ __forceinline__ int lds_word(int e) { return e + (e >> 6); }

__global__ __launch_bounds__(PV_PSOLA_THREADS) void pv_psola_kernel(PvPsolaParams p)
{
    extern __shared__ float4 lds4[];
    float *xs = (float *)lds4;
    float *P = xs + pv_psola_span_words(p.span);
    float *Hn = P + PV_VARI_TABLE_WORDS;
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int mp = p.max_period, span = p.span;
    const int first = (int)blockIdx.x * PV_PSOLA_TILE;           // the tile's first output, relative to the call
    const int cnt = min(PV_PSOLA_TILE, p.nout - first);
    const int j0 = p.out_first + first;                          // its buffer position
    const int r0 = j0 - mp - PV_PSOLA_TAPS / 2;                  // buffer position of span sample e = 0

    // ---- stage: e -> buffer position r0 + e; in[.. - in_first] where the input has it, zero elsewhere
    const float *in_c = p.in + (long)ch * p.in_stride;
    const int e_in0 = min(span, max(0, p.in_first - r0));
    const int e_in1 = max(e_in0, min(span, p.in_first + p.in_count - r0));
    for (int e = tid; e < e_in0; e += PV_PSOLA_THREADS) xs[lds_word(e)] = 0.0f;
    for (int e = e_in1 + tid; e < span; e += PV_PSOLA_THREADS) xs[lds_word(e)] = 0.0f;
    if (e_in1 > e_in0) {
        const int g0 = r0 - p.in_first;                          // in_c index of e = 0; g0 + e >= 0 for e >= e_in0
        const int mis = (int)((((uintptr_t)in_c >> 2) + (uintptr_t)(long)(g0 + e_in0)) & 3);      // in_c + g0 + e_in0 - mis is 16-byte aligned
        const int base = e_in0 - mis;
        const int quads = (e_in1 - base + 3) >> 2;
        for (int q = tid; q < quads; q += PV_PSOLA_THREADS) {
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
        for (int k = tid; k < PV_VARI_TABLE_WORDS / 4; k += PV_PSOLA_THREADS) ((float4 *)P)[k] = g4[k];
        const float4 *h4 = (const float4 *)p.htable;
        for (int k = tid; k < PV_PSOLA_WINDOW_WORDS / 4; k += PV_PSOLA_THREADS) ((float4 *)Hn)[k] = h4[k];
    }
    __syncthreads();

    const int2 tg = p.tile_grains[blockIdx.x];
    const int4 *__restrict__ grains = p.grains;
    float *out = p.out + (long)ch * p.out_stride + first;
    for (int k = 0; k < PV_PSOLA_R; k++) {
        const int nrel = min(tid + k * PV_PSOLA_THREADS, cnt - 1);       // a thread past the tile's end repeats its last output and stores nothing
        const int n = j0 + nrel;
        float num = 0.0f, den = 0.0f;
        bool covered = false;
        for (int g = tg.x; g < tg.y; g++) {
            const int4 G = grains[g];                                    // {t, tf, dq, L}: the same for every lane
            const int L = min(max(G.w, 2), PV_PSOLA_MAX_PERIOD);
            const int dn = min(max(n - G.x, -(1 << 20)), 1 << 20);       // inside +-(tile + max_period + 1) for a range the host made
            const int ua = abs(PV_PSOLA_Q * dn - G.y);
            if (ua >= PV_PSOLA_Q * L) continue;
            const unsigned u4 = 4u * (unsigned)ua;                       // < 2^22
            const unsigned q = u4 / (unsigned)L, rem = u4 - q * (unsigned)L;
            const int qc = (int)min(q, 1024u);
            const float h0 = Hn[qc], h1 = Hn[qc + 1];
            const float h = fmaf((float)rem * (1.0f / (float)L), h1 - h0, h0);
            if (h == 0.0f) continue;
            const int D = G.z >> 8, phi = G.z & (PV_PSOLA_Q - 1);        // floored
            float xt;
            if (phi == 0) {                                              // uniform
                xt = xs[lds_word(min(max(nrel + mp + PV_PSOLA_TAPS / 2 - D, 0), span - 1))];
            } else {
                const int theta = PV_PSOLA_Q - phi;
                const int eb = min(max(nrel + mp - D, 0), span - PV_PSOLA_TAPS);
                float a = 0.0f, s = 0.0f;
#pragma unroll 8
                for (int i = 0; i < PV_PSOLA_TAPS; i++) {
                    const float w = P[abs(PV_PSOLA_Q * (i - (PV_PSOLA_TAPS / 2 - 1)) - theta)];       // at most 32 Q - 1: inside the table
                    a = fmaf(w, xs[lds_word(eb + i)], a);
                    s += w;
                }
                xt = a / s;
            }
            num = fmaf(h, xt, num);
            den += h;
            covered = true;
        }
        if (tid + k * PV_PSOLA_THREADS < cnt) out[nrel] = covered ? num / den : 0.0f;
    }
}

std::atomic<bool> g_lds_psola[16];

}  // namespace

hipError_t pv_launch_psola(const PvPsolaParams &p, hipStream_t stream)
{
    if (p.nout <= 0 || p.nch <= 0) return hipSuccess;
    if (p.max_period < 2 || p.max_period > PV_PSOLA_MAX_PERIOD || p.span != pv_psola_span(p.max_period) || p.nch > 65535) return hipErrorInvalidValue;
    const hipError_t e = pv_set_dynamic_lds_once(g_lds_psola, (const void *)pv_psola_kernel, (int)pv_psola_lds_bytes(PV_PSOLA_MAX_PERIOD));
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((p.nout + PV_PSOLA_TILE - 1) / PV_PSOLA_TILE), (unsigned)p.nch);
    hipLaunchKernelGGL(pv_psola_kernel, grid, dim3(PV_PSOLA_THREADS), pv_psola_lds_bytes(p.max_period), stream, p);
    return hipGetLastError();
}
