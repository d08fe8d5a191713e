// pv_host_common.h -- what the host sides of the fourteen handle types (psola/pv_formant_capi.hip, psola/pv_mirror_capi.hip, pv_capi.hip, stretch/pv_stretch_capi.hip, stretch/pv_f0_capi.hip, resample/pv_resample_capi.hip,
// resample/pv_pitch_capi.hip, resample/pv_vari_capi.hip, resample/pv_glide_capi.hip, psola/pv_psola_capi.hip, psola/pv_epoch_capi.hip, psola/pv_tsm_capi.hip, psola/pv_harmony_capi.hip, psola/pv_takes_capi.hip) share: error reporting, the liveness check, the HIP check macros, the device buffer that grows on demand and the
// twiddle / window tables.  Host code only; everything here is generic over the handle struct H, which has `magic`, `err` and `stream` members.
// It lives in host/ so that the identity of the kernel sources (every *.hip and *.h directly in csrc/, bench.py) does not move with a host-only edit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>
#include <vector>

#include "../../../include/phaze_amd.h"

namespace {

// One specialisation per handle type (PV_HOST_HANDLE, once in its file): its magic word, its destroy entry point, and the thread-local buffer that
// holds the error of a failed create, where no handle exists yet (as large as the handle's own `err`).  The buffers are independent of each
// other.  kNoHandle is what a create function passes to fail / failf to report there.
template <class H> struct HostTraits;

#define PV_HOST_HANDLE(H, MAGIC, DESTROY)                                                                            \
    constexpr H *kNoHandle = nullptr;                                                                                \
    template <> struct HostTraits<H> {                                                                               \
        static constexpr uint32_t kMagic = (MAGIC);                                                                  \
        static constexpr size_t kErrSize = sizeof(H::err);                                                           \
        static int destroy(H *h) { return DESTROY(h); }                                                              \
        static char *create_err() { static thread_local char buf[sizeof(H::err)] = ""; return buf; }                 \
    }

template <class H> bool live(const H *h) { return h && h->magic == HostTraits<H>::kMagic; }

template <class H> const char *last_error(const H *h) { return live(h) ? h->err : HostTraits<H>::create_err(); }

// Every failure goes through here: the message lands in the handle, or with h == nullptr (kNoHandle) in H's create buffer.
template <class H> __attribute__((format(printf, 3, 4))) int failf(H *h, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(h ? h->err : HostTraits<H>::create_err(), HostTraits<H>::kErrSize, fmt, ap);
    va_end(ap);
    return code;
}

template <class H> int fail(H *h, int code, const char *msg) { return failf(h, code, "%s", msg); }

template <class H> int fail_hip(H *h, hipError_t e, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    return fail(h, PV_ERR_DEVICE, buf);
}

#define HIPCHK(h, call)                                            \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) return fail_hip((h), e_, #call);     \
    } while (0)

// Inside a create function, once the handle h exists: a failed call destroys the half-built handle and reports through the create buffer.
#define CREATE_CHK(h, call)                                                \
    do {                                                                   \
        hipError_t e2_ = (call);                                           \
        if (e2_ != hipSuccess) {                                           \
            using H_ = typename std::remove_pointer<decltype(h)>::type;    \
            int rc_ = fail_hip<H_>(nullptr, e2_, #call);                   \
            HostTraits<H_>::destroy(h);                                    \
            return rc_;                                                    \
        }                                                                  \
    } while (0)

// Grows a device buffer to `words` elements (*cap counts elements), contents not kept.  A launch in flight may still use the old buffer: the
// handle's stream is waited for before it is freed.
template <class H, class T> int grow(H *h, T **buf, size_t *cap, size_t words)
{
    if (words <= *cap) return PV_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *cap = 0;
    HIPCHK(h, hipMalloc(buf, words * sizeof(T)));
    *cap = words;
    return PV_OK;
}

// Allocates and fills the tables every transform kernel reads: twiddles exp(-2 pi j k / N) in fp64 and fp32 (role of bundle:12-18) and the periodic
// Hann window (pv:8-14), computed in fp64 on the host, exact on the axes (libm returns ~1e-16 residues there).  half_window: the window is
// followed by N more floats, half of it (exact), for kernels that fold the 1/2 of the split pass into it.  On failure the caller's destroy
// frees what has been allocated.
inline hipError_t upload_tables(int N, bool half_window, double2 **d_tw64, float2 **d_tw32, float **d_hann)
{
    std::vector<double2> tw64(N);
    std::vector<float2> tw32(N);
    std::vector<float> hann(N);
    for (int k = 0; k < N; k++) {
        const double ang = 2.0 * M_PI * (double)k / (double)N;
        tw64[k] = double2{cos(ang), -sin(ang)};
        hann[k] = (float)(0.5 * (1.0 - cos(ang)));
    }
    tw64[0] = double2{1, 0};
    if (N >= 4) { tw64[N / 4] = double2{0, -1}; tw64[3 * N / 4] = double2{0, 1}; }
    tw64[N / 2] = double2{-1, 0};
    for (int k = 0; k < N; k++) tw32[k] = float2{(float)tw64[k].x, (float)tw64[k].y};
    hipError_t e = hipMalloc(d_tw64, sizeof(double2) * N);
    if (e == hipSuccess) e = hipMalloc(d_tw32, sizeof(float2) * N);
    if (e == hipSuccess) e = hipMalloc(d_hann, sizeof(float) * N * (half_window ? 2 : 1));
    if (e == hipSuccess) e = hipMemcpy(*d_tw64, tw64.data(), sizeof(double2) * N, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(*d_tw32, tw32.data(), sizeof(float2) * N, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(*d_hann, hann.data(), sizeof(float) * N, hipMemcpyHostToDevice);
    if (e != hipSuccess || !half_window) return e;
    for (int k = 0; k < N; k++) hann[k] *= 0.5f;
    return hipMemcpy(*d_hann + N, hann.data(), sizeof(float) * N, hipMemcpyHostToDevice);
}

}  // namespace
