// pv_device_common.h -- device helpers shared by the wave kernel (N = 1024) and the workgroup kernel (N = 2048..8192).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pv_signal.h"
#include "pv_mul_rounded.h"
#include "pv_pk_math.h"

// Measured on gfx950 (tools/lds_microbench.hip): ds_read2_b64 / ds_read2st64_b64 / ds_read2_b32 occupy the LDS pipe for 8 cycles, twice
// the cost of the two single reads they replace (2 + 2); ds_write2_b64 is neutral.  The SI load/store optimizer forms them wherever
// two reads share a base register (Hann tables, the fp32 transposes), so the kernels opt out of it per function.  The attribute only
// means something to the device pass.
#if defined(__HIP_DEVICE_COMPILE__)
#define PV_NO_DS_MERGE __attribute__((target("no-load-store-opt")))
#else
#define PV_NO_DS_MERGE
#endif

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));   // clang vector type (the nontemporal builtins need one)

template <typename T> struct v2t;
template <> struct v2t<float> { using type = float2; };
template <> struct v2t<double> { using type = double2; };

template <typename T2> __device__ __forceinline__ T2 cadd(T2 a, T2 b) { return T2{a.x + b.x, a.y + b.y}; }
template <typename T2> __device__ __forceinline__ T2 csub(T2 a, T2 b) { return T2{a.x - b.x, a.y - b.y}; }
template <typename T2> __device__ __forceinline__ T2 cmul(T2 a, T2 b) { return T2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <typename T2> __device__ __forceinline__ T2 cconj(T2 a) { return T2{a.x, -a.y}; }
// multiply by -j (forward) or +j (inverse)
template <bool INV, typename T2> __device__ __forceinline__ T2 rot90(T2 a) { return INV ? T2{-a.y, a.x} : T2{a.y, -a.x}; }

// In-register 8-point DFT, natural order in and out.  INV selects exp(+2 pi j nk/8).
template <typename T, bool INV>
__device__ __forceinline__ void radix8(typename v2t<T>::type (&a)[8])
{
    using T2 = typename v2t<T>::type;
    const T h = (T)0.70710678118654752440;
    const T2 b0 = cadd(a[0], a[4]), b4 = csub(a[0], a[4]);
    const T2 b1 = cadd(a[1], a[5]), b5 = csub(a[1], a[5]);
    const T2 b2 = cadd(a[2], a[6]), b6 = csub(a[2], a[6]);
    const T2 b3 = cadd(a[3], a[7]), b7 = csub(a[3], a[7]);
    // odd half: c_n = b_{n+4} * W8^n
    T2 c1, c3;
    if (!INV) { c1 = T2{(b5.x + b5.y) * h, (b5.y - b5.x) * h}; c3 = T2{(b7.y - b7.x) * h, -(b7.x + b7.y) * h}; }
    else      { c1 = T2{(b5.x - b5.y) * h, (b5.x + b5.y) * h}; c3 = T2{-(b7.x + b7.y) * h, (b7.x - b7.y) * h}; }
    const T2 c0 = b4, c2 = rot90<INV>(b6);
    // even outputs: 4-pt DFT of b0..b3
    {
        const T2 e0 = cadd(b0, b2), e1 = csub(b0, b2), e2 = cadd(b1, b3), e3 = rot90<INV>(csub(b1, b3));
        a[0] = cadd(e0, e2); a[4] = csub(e0, e2); a[2] = cadd(e1, e3); a[6] = csub(e1, e3);
    }
    // odd outputs: 4-pt DFT of c0..c3
    {
        const T2 e0 = cadd(c0, c2), e1 = csub(c0, c2), e2 = cadd(c1, c3), e3 = rot90<INV>(csub(c1, c3));
        a[1] = cadd(e0, e2); a[5] = csub(e0, e2); a[3] = cadd(e1, e3); a[7] = csub(e1, e3);
    }
}

// o * exp(-+2 pi j r / 16): the wave-uniform part of the split-pass twiddle (INV = conjugate)
template <typename T, bool INV>
__device__ __forceinline__ typename v2t<T>::type mul_w16(typename v2t<T>::type o, int r)
{
    using T2 = typename v2t<T>::type;
    const T c = (T)0.92387953251128675613, s = (T)0.38268343236508977173, h = (T)0.70710678118654752440;
    T2 w;
    switch (r) {               // r is a compile-time constant at every call site (unrolled loops)
    case 0: return o;
    case 4: return rot90<INV>(o);
    case 1: w = T2{c, -s}; break;
    case 2: w = T2{h, -h}; break;
    case 3: w = T2{s, -c}; break;
    case 5: w = T2{-s, -c}; break;
    case 6: w = T2{-h, -h}; break;
    default: w = T2{-c, -s}; break;
    }
    if (INV) w.y = -w.y;
    return cmul(o, w);
}

// mul_rounded (a * b rounded to fp32 as an operation of its own, pv:55,67): pv_mul_rounded.h

struct WaveSrc {
    const float *in;
    const float *hist;
    int hist_len;
    bool sys = false;      // resident streaming kernel with its input in DEVICE memory (cached in L2) that the host rewrites through the BAR between quanta WITHIN one launch -> system-scope loads
    __device__ __forceinline__ float at(long s) const
    {
        if (s < 0) return hist[s + hist_len];
        return sys ? __hip_atomic_load(in + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : in[s];
    }
};

constexpr unsigned NOROUTE = 0xFFFFFFFFu;        // route = (rotation index << 16) | target bin

// The pairwise test of the f < 1 scatter (pv_wave_kernel.hip: ov = delta_i - delta_{i+1} <= floor(gap / 2) for every pair of neighbouring peaks) cannot
// fail when f >= 2/3: Math.round(x) lies in (x - 1/2, x + 1/2], so ov = gap - (round(p_{i+1} f) - round(p_i f)) < gap (1 - f) + 1 <= gap / 3 + 1, i.e.
// ov <= ceil(gap / 3), and ceil(gap / 3) <= floor(gap / 2) for every gap >= 3 -- which is the least distance of two local maxima over +-2 bins
// (pv:101-110); no peak is dropped in that range either (pv:127-129).  The kernels skip the test for such f (tests/test_pairwise_rule.py proves the
// bound by exhaustion over peak positions and gaps for N <= 8192).
constexpr float PV_PAIRWISE_SURE = 0.6667f;

// Rotation exp(+2 pi j ridx / N) of one source value (pv:155-170).  R = 4: (delta * t) mod N is a multiple of N/4, so the rotation is
// j^qd exactly: a swap and two sign-bit XORs (j^1 = (-y, x), j^2 = (-x, -y), j^3 = (y, -x)).
template <int R_, int LOG2N_>
__device__ __forceinline__ float2 rotate_route(unsigned route, float2 v, const float2 *__restrict__ tw32)
{
    const unsigned ridx = route >> 16;
    if (R_ == 4) {
        const unsigned qd = (ridx >> (LOG2N_ - 2)) & 3u;                  // bits above the rotation index are don't-care
        const bool sw = (qd & 1u) != 0u;
        const float a = sw ? v.y : v.x, b = sw ? v.x : v.y;
        return float2{__uint_as_float(__float_as_uint(a) ^ ((((qd + 1u) >> 1) & 1u) << 31)), __uint_as_float(__float_as_uint(b) ^ ((qd >> 1) << 31))};
    }
    // v * conj(w), the order of the roundings spelled out: the instances of a kernel (streaming / batch, f >= 1 only / every f) must agree bit for bit,
    // and a contraction left to the compiler comes out as fma(v.x, w.x, v.y * w.y) in one and fma(v.y, w.y, v.x * w.x) in another
    const float2 w = tw32[ridx & ((1u << LOG2N_) - 1u)];                  // masked: NOROUTE carries ridx = 0xFFFF
    return float2{__fmaf_rn(v.x, w.x, __fmul_rn(v.y, w.y)), __fmaf_rn(v.y, w.x, -__fmul_rn(v.x, w.y))};
}
// v * exp(+2 pi j ridx / N) in doubles (rotate_route's fp64 twin: the reference-width flavours)
template <int R_, int LOG2N_>
__device__ __forceinline__ double2 rotate_route_d(unsigned route, double2 v, const double2 *__restrict__ tw64)
{
    const unsigned ridx = (route >> 16) & ((1u << LOG2N_) - 1u);
    if (R_ == 4) { const unsigned q = ridx >> (LOG2N_ - 2); return q == 0 ? v : q == 1 ? double2{-v.y, v.x} : q == 2 ? double2{-v.x, -v.y} : double2{v.y, -v.x}; }   // j^q exactly
    const double2 w = tw64[ridx];                                          // exp(-2 pi j ridx / N): v * conj(w), roundings spelled out (see rotate_route)
    return double2{__fma_rn(v.x, w.x, __dmul_rn(v.y, w.y)), __fma_rn(v.y, w.x, -__dmul_rn(v.x, w.y))};
}

// o * W_32^r = o * exp(-2 pi j r / 32), r = 0..7 (compile-time), fp64: the wave-uniform (row) part of the split-pass twiddle of the 2048- and 8192-point frames
__device__ __forceinline__ double2 mul_w32(double2 o, int r)
{
    constexpr double c[9] = {1.0, 0.98078528040323044913, 0.92387953251128675613, 0.83146961230254523708, 0.70710678118654752440,
                             0.55557023301960222474, 0.38268343236508977173, 0.19509032201612826785, 0.0};
    if (r == 0) return o;
    return cmul(o, double2{c[r], -c[8 - r]});      // sin(2 pi r / 32) = cos(2 pi (8 - r) / 32)
}

// o * exp(+2 pi j r / 32), r = 0..7 (compile-time), packed fp32: the same row part in the c2r twiddle
__device__ __forceinline__ pk::c32 mul_w32_inv_pk(pk::c32 o, int r)
{
    constexpr float c[9] = {1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f, 0.70710678118654752440f,
                            0.55557023301960222474f, 0.38268343236508977173f, 0.19509032201612826785f, 0.0f};
    if (r == 0) return o;
    return pk::cmul(o, pk::c32{c[r], c[8 - r]});
}
// o * exp(+2 pi j r / 16), r = 0..3 (compile-time): the wave-uniform part of the c2r twiddle of the 1024-, 4096- and (eight-element) 8192-point frames, packed
__device__ __forceinline__ pk::c32 mul_w16_inv_pk(pk::c32 o, int r)
{
    const float c = 0.92387953251128675613f, sn = 0.38268343236508977173f, h = 0.70710678118654752440f;
    switch (r) {
    case 0: return o;
    case 1: return pk::cmul(o, pk::c32{c, sn});
    case 2: return pk::mul(pk::add_j(o, o), pk::c32{h, h});
    default: return pk::cmul(o, pk::c32{sn, c});
    }
}

// One conjugate pair of the N = 1024 split pass (FWD) / c2r pass with that factor inside, as ONE asm statement (pk::pair_pass; r compile-time after unrolling)
template <bool FWD, bool SGPR>
__device__ __forceinline__ void pair_pass_w16(int r, pk::c32 a, pk::c32 b, pk::c32 w, pk::c32 s, pk::c32 &x, pk::c32 &y)
{
    const float c = 0.92387953251128675613f, sn = 0.38268343236508977173f, h = 0.70710678118654752440f;
    switch (r) {
    case 0: pk::pair_pass<0, FWD, SGPR>(a, b, w, s, s, x, y); break;       // (no factor: the operand is not named)
    case 1: pk::pair_pass<1, FWD, SGPR>(a, b, w, pk::c32{c, sn}, s, x, y); break;
    case 2: pk::pair_pass<2, FWD, SGPR>(a, b, w, pk::c32{h, h}, s, x, y); break;
    default: pk::pair_pass<3, FWD, SGPR>(a, b, w, pk::c32{sn, c}, s, x, y); break;
    }
}

// base-4 digit reversal over nd digits (fft.js's input order of a radix-4 DIT, bundle:468-508)
__device__ __forceinline__ int digitrev4(int v, int nd)
{
    if (nd == 0) return 0;
    const unsigned r = __brev((unsigned)v) >> (32 - 2 * nd);
    return (int)(((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u));
}

// Register <-> lane transpose WITHOUT LDS: exchanges the register index (8 registers) with the HIGH three lane bits, one bit per stage (see
// pv_wave_fft.h, "transpose 1 of the wave FFTs in registers"); used by the wave FFTs and by transpose 2 of the 8192-point workgroup FFT.
// SELECT (NDW = 2; the fp32-first pitchFactor >= 1 instances of pv_wave_kernel_1024): the last stage without its copies.  A bank-masked DPP move keeps the other lanes
// of its destination, so the compiler copies A first: three instructions per dword pair.  Here A' = (lane bit 3 clear ? A : B[l ^ 8]) is a select with a DPP source into a
// fresh register (v_cndmask_b32_dpp: vcc ? src1 : dpp(src0)), and B' the masked move into B from the A that is still there: two.  Written as asm, four dword pairs a
// statement: the compiler does not know the statement's DPP reads, so the two wait states a DPP read needs behind the VALU write of its source (the permlane swaps of the
// stage before) stand inside it -- the s_mov of the lane mask and one s_nop.
template <int NDW, bool SELECT = false>
__device__ __forceinline__ void transpose_hi3_regs(unsigned (&w)[8][NDW])
{
    static_assert(!SELECT || NDW == 2, "the select form is written for packed fp32 complex elements");
#pragma unroll
    for (int k = 0; k < 4; k++)                       // reg bit 2 <-> lane bit 5
#pragma unroll
        for (int d = 0; d < NDW; d++) {
            const auto r = __builtin_amdgcn_permlane32_swap(w[k][d], w[k + 4][d], false, false);
            w[k][d] = r[0]; w[k + 4][d] = r[1];
        }
#pragma unroll
    for (int q = 0; q < 4; q++) {                     // reg bit 1 <-> lane bit 4
        const int k = (q & 1) | ((q & 2) << 1);       // 0, 1, 4, 5
#pragma unroll
        for (int d = 0; d < NDW; d++) {
            const auto r = __builtin_amdgcn_permlane16_swap(w[k][d], w[k + 2][d], false, false);
            w[k][d] = r[0]; w[k + 2][d] = r[1];
        }
    }
    if constexpr (SELECT) {                           // reg bit 0 <-> lane bit 3
        const unsigned long long keep = 0x00FF00FF00FF00FFull;      // lanes whose bit 3 is clear
#pragma unroll
        for (int k = 0; k < 8; k += 4) {
            unsigned t[4];
#define PV_SEL(T, A, B) "v_cndmask_b32_dpp " T ", " B ", " A ", vcc row_ror:8 row_mask:0xf bank_mask:0xf\n\t"    \
                        "v_mov_b32_dpp " B ", " A " row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
            asm("s_mov_b64 vcc, %12\n\ts_nop 0\n\t" PV_SEL("%0", "%8", "%4") PV_SEL("%1", "%9", "%5") PV_SEL("%2", "%10", "%6") PV_SEL("%3", "%11", "%7")
                : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "+v"(w[k + 1][0]), "+v"(w[k + 1][1]), "+v"(w[k + 3][0]), "+v"(w[k + 3][1])
                : "v"(w[k][0]), "v"(w[k][1]), "v"(w[k + 2][0]), "v"(w[k + 2][1]), "s"(keep)
                : "vcc");
#undef PV_SEL
            w[k][0] = t[0]; w[k][1] = t[1]; w[k + 2][0] = t[2]; w[k + 2][1] = t[3];
        }
    } else
#pragma unroll
    for (int k = 0; k < 8; k += 2)                    // reg bit 0 <-> lane bit 3
#pragma unroll
        for (int d = 0; d < NDW; d++) {
            const unsigned a = w[k][d], b = w[k + 1][d];
            w[k][d] = __builtin_amdgcn_update_dpp(a, b, 0x128, 0xF, 0xC, false);       // lanes 8..15 of every row take B[l ^ 8]
            w[k + 1][d] = __builtin_amdgcn_update_dpp(b, a, 0x128, 0xF, 0x3, false);   // lanes 0..7 take A[l ^ 8]
        }
}

// Wave-local ordering of LDS traffic: LDS instructions of one wave execute in order, so only the compiler must be fenced.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- claim rounds of a workgroup: the colliding scatter of f < 1 frames (pv:169-170; pv_wave_kernel.hip has the story and the one-wave form) ----
// The loop condition is reduced over the workgroup, and -- because several waves race for a claim word here -- a source posts its bin
// with an LDS atomic MIN: the smallest pending source bin wins the round, so every target accumulates its contributions in ascending source order
// (the order of the reference's loops, pv:122,146) whatever the timing of the waves; results are reproducible bit for bit for every f.
// CLAIM[0..H) must be all-ones on entry and is all-ones on exit.
template <int NS, int H_, typename V2>
__device__ __forceinline__ void claim_rounds_wg(const unsigned (&rt)[NS], const V2 (&ys)[NS], const int (&id)[NS], V2 *Y, unsigned *CLAIM)
{
    unsigned pend = 0;
    unsigned tg[NS];
#pragma unroll
    for (int r = 0; r < NS; r++) {
        const unsigned t = rt[r] & 0xFFFFu;
        const bool ok = t < (unsigned)H_;                                  // valid route <=> target field < H
        pend |= ok ? (1u << r) : 0u;
        tg[r] = ok ? t : 0u;
    }
    while (__syncthreads_or(pend != 0u)) {
#pragma unroll
        for (int r = 0; r < NS; r++) if (pend & (1u << r)) atomicMin(&CLAIM[tg[r]], (unsigned)id[r]);
        __syncthreads();
        unsigned c[NS];
        V2 o[NS];
#pragma unroll
        for (int r = 0; r < NS; r++) c[r] = CLAIM[tg[r]];                   // independent reads first, then the winners' stores (see pv_wave_kernel.hip)
#pragma unroll
        for (int r = 0; r < NS; r++) o[r] = Y[tg[r]];
#pragma unroll
        for (int r = 0; r < NS; r++) {
            if ((pend & (1u << r)) && c[r] == (unsigned)id[r]) {
                Y[tg[r]] = V2{o[r].x + ys[r].x, o[r].y + ys[r].y};
                CLAIM[tg[r]] = 0xFFFFFFFFu;                                // only the winner touches the word; losers re-post after the barrier
                pend &= ~(1u << r);
            }
        }
    }
}

// ---- the poll of the resident (streaming) instances: wait for the next quantum's control word in pinned host memory ----
// The word carries the whole quantum -- sequence number (low 16 bits, never 0), channel count (7 bits), ping-pong half (1 bit), timeCursor / hop mod R
// (8 bits) -- so that a successful poll needs no second round trip over PCIe before the input can be requested.  Returns the word behind a system-scope
// acquire fence (what the host wrote before the word), or 0 when the host asks the waves to leave (ctl[4]) or after idle_ticks (~50 ms) without work:
// the host relaunches on demand, a resident wave must never outlive its user.  0 is free for that because a sequence number is never 0 (pv_capi.hip
// skips it when the counter wraps), so no word the host posts is 0; a caller leaves on 0 whichever way it came about.
__device__ __forceinline__ unsigned resident_poll_word(const unsigned *word_at, const unsigned *ctl, unsigned last_seq, unsigned idle_ticks)
{
    unsigned word;
    const unsigned long long idle0 = wall_clock64();
    for (;;) {
        word = __hip_atomic_load(word_at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((word & 0xFFFFu) != (last_seq & 0xFFFFu)) break;
        if (__hip_atomic_load(ctl + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u || wall_clock64() - idle0 > (unsigned long long)idle_ticks) return 0u;
        __builtin_amdgcn_s_sleep(2);
    }
    return word;
}
// one wave per channel slot (N = 1024): every wave polls ctl[0]
__device__ __forceinline__ unsigned resident_poll_wave(const unsigned *ctl, unsigned last_seq, unsigned idle_ticks)
{
    const unsigned word = resident_poll_word(ctl, ctl, last_seq, idle_ticks);
    if (word != 0u) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    return word;
}
// one workgroup per channel slot: thread 0 polls the slot's OWN word ctl[16 + ch] and hands it to the others through `bc`, an LDS word that is not live here
__device__ __forceinline__ unsigned resident_poll_wg(const unsigned *ctl, int ch, unsigned last_seq, unsigned idle_ticks, unsigned *bc, int t)
{
    if (t == 0) bc[0] = resident_poll_word(ctl + 16 + ch, ctl, last_seq, idle_ticks);
    __syncthreads();
    const unsigned word = bc[0];
    __syncthreads();
    if (word != 0u) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    return word;
}

}  // namespace
