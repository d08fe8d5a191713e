// pv_epoch_kernels.hip -- the epoch records (pv_epoch_track), gfx950: a comb of short-time energy steps at the pitch period, on block-scaled integers.
//
// One workgroup per (frame, channel); pv_epoch.h states the record.  Every value written is an exact integer function of the frame's samples and of
// its period, so the reduction order below is free.  The frame is read twice from global memory (the maximum, then the quantised squares: the second
// pass hits the cache) and lives in LDS only as the prefix sums cs[i] = S(0, i) of its squares, wrapping uint32:
//   scan     wave v owns a quarter of the frame and walks it in rows of 64 with a shuffle scan and a carry; the bases of the waves before it are added
//            in a second sweep.  Consecutive lanes touch consecutive words throughout.
//   comb     the candidates phi are strided over the threads; a tooth (phi, k) reads cs at n - w, n and n + w with n = w + phi + ((k p) >> 8), so the
//            lanes of a wave read consecutive words: D = (hi - mid) - (mid - lo), M = (hi - mid) + (mid - lo).
//   pick     argmax of C over phi, ties to the lower phi; the thread that owns phi* stores the record, 16 bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pv_epoch.h"

namespace {

constexpr int EP_TPB = PV_EPOCH_THREADS;
constexpr int EP_WAVES = EP_TPB / 64;

__device__ __forceinline__ unsigned block_umax(unsigned v, unsigned *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned r = red[0];
#pragma unroll
    for (int w = 1; w < EP_WAVES; w++) r = max(r, red[w]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(EP_TPB) void pv_epoch_kernel(PvEpochParams P)
{
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned *cs = (unsigned *)lds;
    unsigned *redu = cs + pv_epoch_prefix_words(P.window);                // 16-byte aligned
    long long *redl = (long long *)(redu + EP_WAVES);
    int *redi = (int *)(redl + EP_WAVES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = P.window;
    const float *x = P.in + (long)blockIdx.y * P.in_stride + (long)blockIdx.x * P.hop;
    int4 *rec = P.rec + (long)blockIdx.y * P.rec_stride + blockIdx.x;
    const int p = P.periods[blockIdx.x];

    // ---- scale -------------------------------------------------------------------------------------------------------------------------
    unsigned amax = 0;
    for (int n = tid; n < W; n += EP_TPB) amax = max(amax, __float_as_uint(x[n]) & 0x7fffffffu);
    amax = block_umax(amax, redu);
    const int w = max(2, p >> 10), Pc = (p + 255) >> 8;
    const int R = W - 2 * w - Pc + 1;                                     // the largest offset of a tooth from the first
    if (amax == 0 || amax >= 0x7f800000u || p < 256 * PV_EPOCH_MIN_PERIOD || p > 256 * P.max_period || R < 0) {   // R >= 0 follows from the create-time ranges
        if (tid == 0) *rec = int4{0, 0, 0, 0};
        return;
    }
    const int ef = (int)(amax >> 23);
    const int e = ef ? ef - 126 : -117 - __clz(amax);                    // A = f 2^e, f in [0.5, 1); a subnormal A = m 2^-149 has e = (32 - clz m) - 149
    const int sh = 10 - e;

    // ---- cs[i] = S(0, i): an inclusive scan of q^2 ------------------------------------------------------------------------------------------
    const int chunk = (W + EP_TPB - 1) / EP_TPB * 64;                     // samples per wave, whole rows of 64
    const int c0 = wave * chunk, c1 = min(c0 + chunk, W);
    unsigned carry = 0;
    for (int i0 = c0; i0 < c1; i0 += 64) {
        const int n = i0 + lane;
        const int q = n < c1 ? (int)rintf(ldexpf(x[n], sh)) : 0;
        unsigned s = (unsigned)(q * q);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = (unsigned)__shfl_up((int)s, off);
            if (lane >= off) s += o;
        }
        s += carry;
        if (n < c1) cs[n + 1] = s;
        carry = (unsigned)__shfl((int)s, 63);
    }
    if (lane == 0) redu[wave] = carry;
    if (tid == 0) cs[0] = 0;
    __syncthreads();
    unsigned base = 0;
#pragma unroll
    for (int v = 0; v < EP_WAVES - 1; v++)
        if (v < wave) base += redu[v];
    for (int n = c0 + lane; n < c1; n += 64) cs[n + 1] += base;
    __syncthreads();

    // ---- comb ----------------------------------------------------------------------------------------------------------------------------
    const int K = (int)(((((long long)R + 1) << 8) - 1) / p) + 1;         // the k with (k p) >> 8 <= R
    constexpr long long NONE = (long long)0x8000000000000000ULL;
    long long myC = NONE, myM = 0;
    int myPhi = 0x7fffffff;
    for (int phi = tid; phi < Pc; phi += EP_TPB) {
        const unsigned *c = cs + w + phi;                                 // c[t] = cs[n] with n = w + phi + t: n - w >= 0 and n + w <= window
        long long C = 0, M = 0;
        for (int k = 0, kp = 0; k < K; k++, kp += p) {                    // kp <= 256 (R + 1) < 2^22
            const int t = kp >> 8;
            const unsigned lo = c[t - w], mid = c[t], hi = c[t + w];
            const unsigned a = hi - mid, b = mid - lo;                    // S(n, n + w) and S(n - w, n), at most 2^29 each
            C += (int)a - (int)b;
            M += a + b;
        }
        if (C > myC) { myC = C; myM = M; myPhi = phi; }                   // phi ascends: the first argmax of this thread's candidates
    }

    // ---- pick: the largest C, then the smallest phi ------------------------------------------------------------------------------------------
    long long bC = myC;
    int bPhi = myPhi;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long oC = __shfl_xor(bC, off);
        const int oPhi = __shfl_xor(bPhi, off);
        if (oC > bC || (oC == bC && oPhi < bPhi)) { bC = oC; bPhi = oPhi; }
    }
    if (lane == 0) { redl[wave] = bC; redi[wave] = bPhi; }
    __syncthreads();
    bC = redl[0]; bPhi = redi[0];
#pragma unroll
    for (int v = 1; v < EP_WAVES; v++) {
        const long long oC = redl[v];
        const int oPhi = redi[v];
        if (oC > bC || (oC == bC && oPhi < bPhi)) { bC = oC; bPhi = oPhi; }
    }
    if (myPhi == bPhi) {                                                  // one thread: every thread with a candidate has its own phi, and Pc >= 8
        const unsigned long long num = (unsigned long long)(myC > 0 ? myC : 0) << 14;      // C <= Mtot < 2^41
        const int s = myM > 0 ? (int)(num / (unsigned long long)myM) : 0;
        *rec = int4{w + bPhi, K, w, s};
    }
}

}  // namespace

hipError_t pv_launch_epoch(const float *in, long in_stride, int nch, int nframes, int window, int hop, int max_period, const int *periods, int *records,
                           long rec_stride, hipStream_t st)
{
    if (max_period < PV_EPOCH_MIN_PERIOD || max_period > PV_EPOCH_MAX_PERIOD || window < 2 * max_period || window > PV_EPOCH_MAX_WINDOW || hop < 1
        || hop > PV_EPOCH_MAX_HOP || nch < 1 || nch > 65535 || nframes < 1 || !in || !periods || !records || ((uintptr_t)records & 15) != 0)
        return hipErrorInvalidValue;
    PvEpochParams p{in, in_stride, periods, (int4 *)records, rec_stride, window, hop, max_period};
    hipLaunchKernelGGL(pv_epoch_kernel, dim3((unsigned)nframes, (unsigned)nch), dim3(EP_TPB), pv_epoch_lds_bytes(window), st, p);
    return hipGetLastError();
}
