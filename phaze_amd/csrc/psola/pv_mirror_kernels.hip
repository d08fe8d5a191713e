// pv_mirror_kernels.hip -- overlap-add of Hann grains that read the input in either time direction, for gfx950: every output sample gathers the grains
// that cover it, and a grain reads the input upwards from n - D or, mirrored, downwards from D - n (contract, arithmetic and summation order:
// pv_mirror.h).
//
// The structure is pv_tsm_kernels.hip's, whose device arithmetic is restated here operation for operation (that file's resource figures are pinned, so
// it stays as it is): one workgroup per (tile of PV_TSM_TILE consecutive outputs, channel) stages the tile's source range [src0, src0 + src_count), the
// prototype table P and the window table Hn in LDS; every thread runs PV_TSM_R outputs, PV_TSM_THREADS apart, so that the 64 lanes of a wave always
// work on 64 consecutive outputs.  A grain record is the same for every lane (a uniform index: scalar loads), the waves a grain does not reach skip it
// as a whole, and the 64 weights of a fractionally displaced grain are broadcast reads of P.  A launch's LDS is sized by the longest source range among
// its tiles (p.span).
// What is new is the direction bit of a record.  It is read with the record, so it is uniform across the wave: a branch that every lane takes the
// same way, not a divergence.  It selects the span index of the lane's output, e0 = n - D - src0 or e0 = D - n - src0; the taps then run upwards from
// e0 - 32 in both cases, with the forward weights (pv_mirror.h), so nothing after e0 knows the direction.
// LDS banks: under a mirrored grain consecutive lanes read consecutive words downwards.  A one-dword LDS read is served in two groups of 32 lanes and
// conflicts only between lanes of a group on one of the 32 banks; the 32 lanes of a group read 32 consecutive samples whichever way the lane index
// runs, that is the same set of words as 32 lanes walking upwards over those samples.  In the padded layout e + (e >> 6) such a set spans 32 or (across
// one padding word) 33 consecutive words: conflict-free, or one pair of lanes on one bank, exactly as for the forward grain.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../pv_kernels.h"
#include "pv_mirror.h"

namespace {

__device__ __forceinline__ int lds_word(int e) { return e + (e >> 6); }

__global__ __launch_bounds__(PV_TSM_THREADS) void pv_mirror_kernel(PvTsmParams p)
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
            const int ua = abs(PV_TSM_Q * dn - (G.y & (PV_TSM_Q - 1)));
            if (ua >= PV_TSM_Q * L) continue;
            const unsigned u4 = 4u * (unsigned)ua;                       // < 2^22
            const unsigned q = u4 / (unsigned)L, rem = u4 - q * (unsigned)L;
            const int qc = (int)min(q, 1024u);
            const float h0 = Hn[qc], h1 = Hn[qc + 1];
            const float h = fmaf((float)rem * (1.0f / (float)L), h1 - h0, h0);
            if (h == 0.0f) continue;
            const int phi = (G.y >> 8) & (PV_TSM_Q - 1);
            // the span index of the position n - D (forward) or D - n (mirrored): in [33, src_count - 32) for a grain that covers n, since the host took
            // it into the tile's range; formed in unsigned arithmetic, since n - D and D - n alone may pass 2^31, and clamped like every LDS index
            const unsigned up = (unsigned)n - (unsigned)G.z, down = (unsigned)G.z - (unsigned)n;
            const int e0 = (int)(((G.y & PV_MIRROR_BIT) ? down : up) - (unsigned)src0);             // uniform choice
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

std::atomic<bool> g_lds_mirror[16];

}  // namespace

hipError_t pv_launch_mirror(const PvTsmParams &p, hipStream_t stream)
{
    if (p.nout <= 0 || p.nch <= 0) return hipSuccess;
    if (p.span < 2 * PV_TSM_TAPS || pv_tsm_lds_bytes(p.span) > PV_TSM_LDS_BYTES || p.nch > 65535 || p.in_count < 0) return hipErrorInvalidValue;
    const hipError_t e = pv_set_dynamic_lds_once(g_lds_mirror, (const void *)pv_mirror_kernel, PV_TSM_LDS_BYTES);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((p.nout + PV_TSM_TILE - 1) / PV_TSM_TILE), (unsigned)p.nch);
    hipLaunchKernelGGL(pv_mirror_kernel, grid, dim3(PV_TSM_THREADS), pv_tsm_lds_bytes(p.span), stream, p);
    return hipGetLastError();
}
