// pv_pk_math.h -- packed-fp32 complex arithmetic for gfx950 (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 with op_sel / neg modifiers).
//
// A complex number lives in one 64-bit VGPR pair (x = low dword, y = high dword).  The VOP3P source modifiers make conjugation,
// multiplication by +-j and the real/imaginary cross terms of a complex product free: op_sel[i] picks the dword of source i that feeds
// the LOW result, op_sel_hi[i] the one that feeds the HIGH result, neg_lo / neg_hi negate source i per result half.  The compiler does
// not fold these swaps (it emits v_mov pairs instead: 66 moves per 512-point FFT), hence the one-instruction asm helpers below.
// They are plain (non-volatile) asm: pure functions of their operands, free to be scheduled, CSE'd or dropped.
#pragma once
#include <hip/hip_runtime.h>

namespace pk {

typedef float c32 __attribute__((ext_vector_type(2)));

#define PV_PK2(name, text)                                                                          \
    __device__ __forceinline__ c32 name(c32 a, c32 b) { c32 d; asm(text : "=v"(d) : "v"(a), "v"(b)); return d; }
#define PV_PK3(name, text)                                                                          \
    __device__ __forceinline__ c32 name(c32 a, c32 b, c32 c) { c32 d; asm(text : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }

PV_PK2(add, "v_pk_add_f32 %0, %1, %2")                                                               // a + b
PV_PK2(sub, "v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]")                                     // a - b
PV_PK2(add_j, "v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]")                   // a + j b = (ax - by, ay + bx)
PV_PK2(sub_j, "v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]")                   // a - j b = (ax + by, ay - bx)
PV_PK2(add_conj, "v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]")                                             // a + conj(b)
PV_PK2(sub_conj, "v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]")                                             // a - conj(b)
PV_PK2(neg_add_j, "v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[1,1] neg_hi:[1,0]")  // -a + j b = (-ax - by, -ay + bx)
PV_PK2(mul, "v_pk_mul_f32 %0, %1, %2")                                                               // component-wise
PV_PK2(mul_conj, "v_pk_mul_f32 %0, %1, %2 neg_hi:[0,1]")                                             // conj of the component-wise product: (ax bx, -ay by)
PV_PK2(conj_add_j, "v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[1,1]") // conj(a + j b) = (ax - by, -ay - bx)
PV_PK2(mul_ay, "v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[1,0]")                  // (-ay by, ay bx)
PV_PK3(fma_ax, "v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]")                       // (ax bx + cx, ax by + cy)
PV_PK3(fma, "v_pk_fma_f32 %0, %1, %2, %3")                                                           // a * b + c component-wise
PV_PK3(fnma, "v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[1,0,0] neg_hi:[1,0,0]")                            // -a * b + c
PV_PK3(fma_j, "v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]")         // c + j (a * b)  (b = (s, s))
PV_PK3(fnma_j, "v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]")        // c - j (a * b)  (b = (s, s))
PV_PK3(conj_fma_j, "v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,1]")   // conj(c + j (a * b)) = (cx - ay s, -cy - ax s)  (b = (s, s))
PV_PK3(fms, "v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]")                             // a * b - c component-wise
PV_PK3(fma_addj, "v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,1,0] neg_lo:[0,0,1]")      // a * b + j c
PV_PK3(fma_conj_subj, "v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,1,0] neg_hi:[1,0,0]") // conj(a * b - j c) = (ax bx + cy, -ay by + cx)  (b = (s, s))

#undef PV_PK2
#undef PV_PK3

// a * w (complex): two instructions
__device__ __forceinline__ c32 cmul(c32 a, c32 w) { return fma_ax(a, w, mul_ay(a, w)); }

// ---- fused forms: several dependent packed instructions in ONE asm statement ----
// The compiler assumes that a register written by an asm statement has a forwarding hazard and pads its first read with an s_nop unless an instruction it can see
// into stands in between -- and in its count of wait states asm statements are worth nothing: a run of one-instruction helpers takes a pad at every level of its
// dependency tree (91 wait states per N = 1024 frame, profiles/frame_copies_parent.md).  Packed fp32 -> packed fp32 needs no wait state, so the chains below are written
// out in one string each; the instructions, their operands and their order are those of the helpers above: the same bits.  Results that an instruction writes while
// inputs of the statement are still to be read are early-clobber ("=&v"); a "+v" operand is consumed in place.  TRIM bit 1 (TRIM_SGPR): the wave-uniform factor comes
// as an SGPR pair ("s"; every instruction names at most one: the constant-bus limit of VOP3P on gfx950) instead of being copied into a VGPR pair at every use.
constexpr int TRIM_FUSE = 1, TRIM_SGPR = 2, TRIM_DPP = 4;

#define PV_MUL_AY(d, a, b) "v_pk_mul_f32 " d ", " a ", " b " op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[1,0]\n\t"
#define PV_FMA_AX(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c " op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"
#define PV_ADD(d, a, b) "v_pk_add_f32 " d ", " a ", " b "\n\t"
#define PV_SUB(d, a, b) "v_pk_add_f32 " d ", " a ", " b " neg_lo:[0,1] neg_hi:[0,1]\n\t"
#define PV_ADD_J(d, a, b) "v_pk_add_f32 " d ", " a ", " b " op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]\n\t"
#define PV_SUB_J(d, a, b) "v_pk_add_f32 " d ", " a ", " b " op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]\n\t"
#define PV_NEG_ADD_J(d, a, b) "v_pk_add_f32 " d ", " a ", " b " op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[1,1] neg_hi:[1,0]\n\t"
#define PV_ADD_CONJ(d, a, b) "v_pk_add_f32 " d ", " a ", " b " neg_hi:[0,1]\n\t"
#define PV_SUB_CONJ(d, a, b) "v_pk_add_f32 " d ", " a ", " b " neg_lo:[0,1]\n\t"
#define PV_MUL(d, a, b) "v_pk_mul_f32 " d ", " a ", " b "\n\t"
#define PV_FMA(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c "\n\t"
#define PV_FNMA(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c " neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"
#define PV_FMS(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c " neg_lo:[0,0,1] neg_hi:[0,0,1]\n\t"
#define PV_FMA_J(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c " op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]\n\t"
#define PV_FNMA_J(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c " op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]\n\t"
#define PV_CONJ_FMA_J(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c " op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,1]\n\t"
#define PV_FMA_ADDJ(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c " op_sel:[0,0,1] op_sel_hi:[1,1,0] neg_lo:[0,0,1]\n\t"
#define PV_FMA_CONJ_SUBJ(d, a, b, c) "v_pk_fma_f32 " d ", " a ", " b ", " c " op_sel:[0,0,1] op_sel_hi:[1,1,0] neg_hi:[1,0,0]\n\t"

// cmul in one statement
__device__ __forceinline__ c32 cmul_fused(c32 a, c32 w)
{
    c32 d;
    asm(PV_MUL_AY("%0", "%1", "%2") PV_FMA_AX("%0", "%1", "%2", "%0") : "=&v"(d) : "v"(a), "v"(w));
    return d;
}
template <int TRIM> __device__ __forceinline__ c32 cmul_t(c32 a, c32 w) { if constexpr (TRIM & TRIM_FUSE) return cmul_fused(a, w); else return cmul(a, w); }

// One conjugate pair of the split pass (FWD) / the c2r pass (!FWD), one statement of 6 + (0, 2, 2, 2 for R = 0 .. 3) instructions: with E = a + conj(b), O = a - conj(b),
// T = (O * exp(+2 pi j R / 16)) * w:   FWD: x = conj(E + j T s), y = E - j T s;   !FWD: x = E s + j T, y = conj(E s - j T)   (s = (sc, sc)).  w16 is the wave-uniform
// factor of R = 1, 3 (cos, sin) resp. R = 2 (h, h) (unused for R = 0).  What the one-instruction helpers compute, in their order.
template <int R, bool FWD, bool SGPR>
__device__ __forceinline__ void pair_pass(c32 a, c32 b, c32 w, c32 w16, c32 s, c32 &x, c32 &y)
{
    c32 e, o, p;
#define PV_PAIR_TEXT(W16, S)                                                                                                                        \
    PV_ADD_CONJ("%0", "%3", "%4") PV_SUB_CONJ("%1", "%3", "%4")                                                                                     \
    W16                                                                                                                                             \
    PV_MUL_AY("%2", "%1", "%5") PV_FMA_AX("%1", "%1", "%5", "%2")                                                                                   \
    S
#define PV_PAIR_R0 ""
#define PV_PAIR_R13 PV_MUL_AY("%2", "%1", "%6") PV_FMA_AX("%1", "%1", "%6", "%2")
#define PV_PAIR_R2 PV_ADD_J("%1", "%1", "%1") PV_MUL("%1", "%1", "%6")
#define PV_PAIR_FWD PV_CONJ_FMA_J("%2", "%1", "%7", "%0") PV_FNMA_J("%0", "%1", "%7", "%0")
#define PV_PAIR_INV PV_FMA_ADDJ("%2", "%0", "%7", "%1") PV_FMA_CONJ_SUBJ("%0", "%0", "%7", "%1")
#define PV_PAIR_ASM(W16, S)                                                                                                                         \
    if constexpr (SGPR) asm(PV_PAIR_TEXT(W16, S) : "=&v"(e), "=&v"(o), "=&v"(p) : "v"(a), "v"(b), "v"(w), "s"(w16), "s"(s));                         \
    else asm(PV_PAIR_TEXT(W16, S) : "=&v"(e), "=&v"(o), "=&v"(p) : "v"(a), "v"(b), "v"(w), "v"(w16), "v"(s))
    if constexpr (FWD) {
        if constexpr (R == 0) { PV_PAIR_ASM(PV_PAIR_R0, PV_PAIR_FWD); }
        else if constexpr (R == 2) { PV_PAIR_ASM(PV_PAIR_R2, PV_PAIR_FWD); }
        else { PV_PAIR_ASM(PV_PAIR_R13, PV_PAIR_FWD); }
    } else {
        if constexpr (R == 0) { PV_PAIR_ASM(PV_PAIR_R0, PV_PAIR_INV); }
        else if constexpr (R == 2) { PV_PAIR_ASM(PV_PAIR_R2, PV_PAIR_INV); }
        else { PV_PAIR_ASM(PV_PAIR_R13, PV_PAIR_INV); }
    }
#undef PV_PAIR_ASM
#undef PV_PAIR_INV
#undef PV_PAIR_FWD
#undef PV_PAIR_R2
#undef PV_PAIR_R13
#undef PV_PAIR_R0
#undef PV_PAIR_TEXT
    x = p; y = e;
}

// (c - n)^2 - (c + n) (K + R (c + n)) of the guard band (pv_guard.h), five instructions in one statement; K from an SGPR pair if SGPR
template <bool SGPR>
__device__ __forceinline__ c32 band_test(c32 c, c32 n, c32 rr, c32 kk)
{
    c32 d, s, t;
#define PV_BAND_TEXT PV_SUB("%0", "%3", "%4") PV_ADD("%1", "%3", "%4") PV_FMA("%2", "%1", "%5", "%6") PV_MUL("%1", "%2", "%1") PV_FMS("%0", "%0", "%0", "%1")
    if constexpr (SGPR) asm(PV_BAND_TEXT : "=&v"(d), "=&v"(s), "=&v"(t) : "v"(c), "v"(n), "v"(rr), "s"(kk));
    else asm(PV_BAND_TEXT : "=&v"(d), "=&v"(s), "=&v"(t) : "v"(c), "v"(n), "v"(rr), "v"(kk));
#undef PV_BAND_TEXT
    return d;
}

// In-register 8-point inverse DFT (exp(+2 pi j nk/8)), natural order in and out: 26 packed instructions.
__device__ __forceinline__ void radix8_inv(c32 (&a)[8])
{
    const c32 hh{0.70710678118654752440f, 0.70710678118654752440f};
    const c32 b0 = add(a[0], a[4]), b4 = sub(a[0], a[4]);
    const c32 b1 = add(a[1], a[5]), b5 = sub(a[1], a[5]);
    const c32 b2 = add(a[2], a[6]), b6 = sub(a[2], a[6]);
    const c32 b3 = add(a[3], a[7]), b7 = sub(a[3], a[7]);
    {   // even outputs: 4-point DFT of b0..b3
        const c32 e0 = add(b0, b2), e1 = sub(b0, b2), e2 = add(b1, b3), t = sub(b1, b3);
        a[0] = add(e0, e2); a[4] = sub(e0, e2); a[2] = add_j(e1, t); a[6] = sub_j(e1, t);
    }
    {   // odd outputs: 4-point DFT of c_n = b_{n+4} W8^{-n}; c1 = h u1, c3 = h u3 with the factor h folded into the last stage
        const c32 u1 = add_j(b5, b5);          // b5 (1 + j)
        const c32 u3 = neg_add_j(b7, b7);      // b7 (-1 + j)
        const c32 e0 = add_j(b4, b6), e1 = sub_j(b4, b6);
        const c32 e2 = add(u1, u3), t = sub(u1, u3);
        a[1] = fma(e2, hh, e0); a[5] = fnma(e2, hh, e0); a[3] = fma_j(t, hh, e1); a[7] = fnma_j(t, hh, e1);
    }
}

// radix8_inv in six statements instead of twenty-six: the four first-stage butterflies one each (a butterfly waits for its own two inputs only: the transposes' reads
// land one by one), then the even and the odd half of the second and third stage in one statement each, computed in place on their four inputs and one more pair:
//     even:  t = b0 + b2 | b2 = b0 - b2 (e1) | b0 = b1 + b3 (e2) | b3 = b1 - b3 | b1 = t + b0 (a0) | t = t - b0 (a4) | b0 = b2 + j b3 (a2) | b2 = b2 - j b3 (a6)
//     odd:   b5 = b5 (1 + j) | b7 = b7 (-1 + j) | t = b4 + j b6 (e0) | b6 = b4 - j b6 (e1) | b4 = b5 + b7 (e2) | b5 = b5 - b7 | b7 = b4 h + t (a1) | t = -b4 h + t (a5)
//            | b4 = e1 + j b5 h (a3) | b6 = e1 - j b5 h (a7)
template <bool SGPR>
__device__ __forceinline__ void radix8_inv_fused(c32 (&a)[8])
{
    const c32 hh{0.70710678118654752440f, 0.70710678118654752440f};
    c32 b[8], t;
#pragma unroll
    for (int k = 0; k < 4; k++) asm(PV_ADD("%0", "%2", "%3") PV_SUB("%1", "%2", "%3") : "=&v"(b[k]), "=v"(b[k + 4]) : "v"(a[k]), "v"(a[k + 4]));
    asm(PV_ADD("%4", "%0", "%2") PV_SUB("%2", "%0", "%2") PV_ADD("%0", "%1", "%3") PV_SUB("%3", "%1", "%3")
        PV_ADD("%1", "%4", "%0") PV_SUB("%4", "%4", "%0") PV_ADD_J("%0", "%2", "%3") PV_SUB_J("%2", "%2", "%3")
        : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "=&v"(t));
    a[0] = b[1]; a[4] = t; a[2] = b[0]; a[6] = b[2];
#define PV_ODD_TEXT                                                                                                                                 \
    PV_ADD_J("%1", "%1", "%1") PV_NEG_ADD_J("%3", "%3", "%3") PV_ADD_J("%4", "%0", "%2") PV_SUB_J("%2", "%0", "%2") PV_ADD("%0", "%1", "%3")          \
    PV_SUB("%1", "%1", "%3") PV_FMA("%3", "%0", "%5", "%4") PV_FNMA("%4", "%0", "%5", "%4") PV_FMA_J("%0", "%1", "%5", "%2") PV_FNMA_J("%2", "%1", "%5", "%2")
    if constexpr (SGPR) asm(PV_ODD_TEXT : "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]), "=&v"(t) : "s"(hh));
    else asm(PV_ODD_TEXT : "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]), "=&v"(t) : "v"(hh));
#undef PV_ODD_TEXT
    a[1] = b[7]; a[5] = t; a[3] = b[4]; a[7] = b[6];
}
template <int TRIM> __device__ __forceinline__ void radix8_inv_t(c32 (&a)[8])
{
    if constexpr (TRIM & TRIM_FUSE) radix8_inv_fused<(TRIM & TRIM_SGPR) != 0>(a); else radix8_inv(a);
}

}  // namespace pk
