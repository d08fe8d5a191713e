// pv_f0_capi.hip -- the pv_f0_* entry points of include/phaze_amd.h: the fundamental-frequency tracker (kernel: pv_f0_kernels.hip).
//
// A pv_f0 holds a geometry (window, hop, lag range) and the staging buffers of the host-pointer form; the tracker itself carries no state from
// call to call.  pv_f0_period and pv_tune_plan, the host code that consumes the records, are in pv_tune_plan.hip.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../host/pv_host_common.h"
#include "pv_stretch.h"

struct pv_f0 {
    uint32_t magic;
    int W, hop, min_lag, max_lag, max_channels, max_frames, device;
    hipStream_t own_stream, stream;
    float *d_in;                             // host-pointer calls: one piece of input, [max_channels][(max_frames - 1) hop + W + max_lag]
    int32_t *d_rec;                          // and its records, [max_channels][max_frames][4]
    char err[384];
};

namespace {

PV_HOST_HANDLE(pv_f0, 0x50564630u /* 'PVF0' */, pv_f0_destroy);

int64_t span(const pv_f0 *h, int64_t nframes) { return (nframes - 1) * h->hop + h->W + h->max_lag; }

// What both forms check before any device work.
int check(pv_f0 *h, const char *fn, const void *in, const void *records, int32_t nch, int64_t nframes, int64_t in_stride, int32_t threshold, int64_t rec_stride)
{
    if (nch < 0 || nframes < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel or frame count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (threshold < 1 || threshold > 16384) return failf(h, PV_ERR_ARGUMENT, "%s: threshold %d is outside [1, 16384] (units of 2^-14)", fn, (int)threshold);
    if (nframes > 0x7fffffff) return failf(h, PV_ERR_ARGUMENT, "%s: more than 2^31 - 1 frames in one call", fn);
    if (nch == 0 || nframes == 0) return PV_OK;
    if (!in || !records) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch > 1 && (in_stride < span(h, nframes) || rec_stride < nframes))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the %lld samples read and the %lld records written per channel", fn,
                     (long long)span(h, nframes), (long long)nframes);
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_f0_last_error(const pv_f0 *h) { return last_error(h); }

int pv_f0_destroy(pv_f0 *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->d_in) (void)hipFree(h->d_in);
    if (h->d_rec) (void)hipFree(h->d_rec);
    (void)hipGetLastError();
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_f0_create(const pv_f0_config *cfg, pv_f0 **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_f0_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_f0_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_f0_create: pv_f0_config.struct_size does not match this library (start from PV_F0_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_f0_create: unknown bits in pv_f0_config.flags (must be 0)");
    if (cfg->window < 16 || cfg->window > 4096) return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_f0_create: window %d is outside [16, 4096]", (int)cfg->window);
    if (cfg->hop < 1 || cfg->hop > 4096) return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_f0_create: hop %d is outside [1, 4096]", (int)cfg->hop);
    if (cfg->min_lag < 2 || cfg->min_lag >= cfg->max_lag || cfg->max_lag > 4096)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_f0_create: lags [%d, %d] must satisfy 2 <= min_lag < max_lag <= 4096", (int)cfg->min_lag, (int)cfg->max_lag);
    if (cfg->max_channels < 0 || cfg->max_channels > 65535)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_f0_create: max_channels %d is outside [0, 65535]", (int)cfg->max_channels);
    if (cfg->max_frames < 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_f0_create: negative max_frames");

    pv_f0 *h = (pv_f0 *)calloc(1, sizeof(pv_f0));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_f0_create: out of host memory");
    h->magic = HostTraits<pv_f0>::kMagic;
    h->W = cfg->window; h->hop = cfg->hop; h->min_lag = cfg->min_lag; h->max_lag = cfg->max_lag;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    h->max_frames = cfg->max_frames > 0 ? cfg->max_frames : 256;
    h->device = cfg->device_id;
    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    CREATE_CHK(h, hipMalloc(&h->d_in, sizeof(float) * (size_t)h->max_channels * (size_t)span(h, h->max_frames)));
    CREATE_CHK(h, hipMalloc(&h->d_rec, sizeof(int32_t) * 4 * (size_t)h->max_channels * (size_t)h->max_frames));
    *out = h;
    return PV_OK;
}

int pv_f0_set_stream(pv_f0 *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_f0_set_stream: hipStreamSynchronize failed");
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_f0_synchronize(pv_f0 *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_f0_synchronize: hipStreamSynchronize failed");
    return PV_OK;
}

int pv_f0_track_device(pv_f0 *h, const float *d_in, int32_t nch, int64_t nframes, int64_t in_stride, int32_t threshold, int32_t *d_records, int64_t rec_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check(h, "pv_f0_track_device", d_in, d_records, nch, nframes, in_stride, threshold, rec_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    if (((uintptr_t)d_records & 15) != 0) return fail(h, PV_ERR_ARGUMENT, "pv_f0_track_device: records must be 16-byte aligned (one store per record)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, pv_launch_f0(d_in, (long)in_stride, nch, (int)nframes, h->W, h->hop, h->min_lag, h->max_lag, threshold, d_records, (long)rec_stride, h->stream));
    return PV_OK;
}

int pv_f0_track(pv_f0 *h, const float *in, int32_t nch, int64_t nframes, int64_t in_stride, int32_t threshold, int32_t *records, int64_t rec_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check(h, "pv_f0_track", in, records, nch, nframes, in_stride, threshold, rec_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t piece_span = span(h, h->max_frames);
    for (int64_t m0 = 0; m0 < nframes; m0 += h->max_frames) {           // pieces of max_frames frames; a piece re-reads the W + max_lag - hop samples it shares
        const int64_t F = nframes - m0 < h->max_frames ? nframes - m0 : h->max_frames;
        const size_t row = sizeof(float) * (size_t)span(h, F);
        HIPCHK(h, hipMemcpy2DAsync(h->d_in, sizeof(float) * (size_t)piece_span, in + m0 * h->hop, sizeof(float) * (size_t)(nch > 1 ? in_stride : span(h, F)), row,
                                   nch, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, pv_launch_f0(h->d_in, (long)piece_span, nch, (int)F, h->W, h->hop, h->min_lag, h->max_lag, threshold, h->d_rec, h->max_frames, h->stream));
        const size_t rrow = 16 * (size_t)F;
        HIPCHK(h, hipMemcpy2DAsync(records + 4 * m0, 16 * (size_t)(nch > 1 ? rec_stride : F), h->d_rec, 16 * (size_t)h->max_frames, rrow, nch, hipMemcpyDeviceToHost,
                                   h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PV_OK;
}

}  // extern "C"
