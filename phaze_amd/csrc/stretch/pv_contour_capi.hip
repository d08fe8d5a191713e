// pv_contour_capi.hip -- the pv_contour_* handle entry points of include/phaze_amd.h: the candidate tables of the pitch contour tracker (kernel:
// pv_contour_kernels.hip).
//
// A pv_contour holds a geometry (window, hop, lag range, candidates per frame) and the staging buffers of the host-pointer form; it carries no state from
// call to call.  pv_contour_path, the host code that turns a table into f0 records, is in pv_contour_path.hip.  This file mirrors pv_f0_capi.hip: the same
// checks in the same order, with the bias in the place of the threshold.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../host/pv_host_common.h"
#include "pv_contour.h"

struct pv_contour {
    uint32_t magic;
    int W, hop, min_lag, max_lag, K, max_channels, max_frames, device;
    hipStream_t own_stream, stream;
    float *d_in;                             // host-pointer calls: one piece of input, [max_channels][(max_frames - 1) hop + W + max_lag]
    int32_t *d_cand;                         // and its tables, [max_channels][max_frames][K][4]
    char err[384];
};

namespace {

PV_HOST_HANDLE(pv_contour, 0x50564354u /* 'PVCT' */, pv_contour_destroy);

int64_t span(const pv_contour *h, int64_t nframes) { return (nframes - 1) * h->hop + h->W + h->max_lag; }

// What both forms check before any device work.
int check(pv_contour *h, const char *fn, const void *in, const void *cand, int32_t nch, int64_t nframes, int64_t in_stride, int32_t bias, int64_t cand_stride)
{
    if (nch < 0 || nframes < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel or frame count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (bias < 0 || bias > PV_CONTOUR_MAX_BIAS) return failf(h, PV_ERR_ARGUMENT, "%s: bias %d is outside [0, 16384] (units of 2^-14 over the lag range)", fn, (int)bias);
    if (nframes > 0x7fffffff) return failf(h, PV_ERR_ARGUMENT, "%s: more than 2^31 - 1 frames in one call", fn);
    if (nch == 0 || nframes == 0) return PV_OK;
    if (!in || !cand) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch > 1 && (in_stride < span(h, nframes) || cand_stride < nframes))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the %lld samples read and the %lld frames written per channel", fn,
                     (long long)span(h, nframes), (long long)nframes);
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_contour_last_error(const pv_contour *h) { return last_error(h); }

int pv_contour_destroy(pv_contour *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->d_in) (void)hipFree(h->d_in);
    if (h->d_cand) (void)hipFree(h->d_cand);
    (void)hipGetLastError();
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_contour_create(const pv_contour_config *cfg, pv_contour **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_contour_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: pv_contour_config.struct_size does not match this library (start from PV_CONTOUR_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: unknown bits in pv_contour_config.flags (must be 0)");
    if (cfg->window < 16 || cfg->window > 4096) return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: window %d is outside [16, 4096]", (int)cfg->window);
    if (cfg->hop < 1 || cfg->hop > 4096) return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: hop %d is outside [1, 4096]", (int)cfg->hop);
    if (cfg->min_lag < 2 || cfg->min_lag >= cfg->max_lag || cfg->max_lag > 4096)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: lags [%d, %d] must satisfy 2 <= min_lag < max_lag <= 4096", (int)cfg->min_lag, (int)cfg->max_lag);
    if (cfg->candidates < 0 || cfg->candidates > PV_CONTOUR_MAX_CANDIDATES)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: candidates %d is outside [0, 8] (0 selects 8)", (int)cfg->candidates);
    if (cfg->max_channels < 0 || cfg->max_channels > 65535)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: max_channels %d is outside [0, 65535]", (int)cfg->max_channels);
    if (cfg->max_frames < 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_contour_create: negative max_frames");

    pv_contour *h = (pv_contour *)calloc(1, sizeof(pv_contour));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_contour_create: out of host memory");
    h->magic = HostTraits<pv_contour>::kMagic;
    h->W = cfg->window; h->hop = cfg->hop; h->min_lag = cfg->min_lag; h->max_lag = cfg->max_lag;
    h->K = cfg->candidates > 0 ? cfg->candidates : PV_CONTOUR_MAX_CANDIDATES;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    h->max_frames = cfg->max_frames > 0 ? cfg->max_frames : 256;
    h->device = cfg->device_id;
    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    CREATE_CHK(h, hipMalloc(&h->d_in, sizeof(float) * (size_t)h->max_channels * (size_t)span(h, h->max_frames)));
    CREATE_CHK(h, hipMalloc(&h->d_cand, sizeof(int32_t) * 4 * (size_t)h->K * (size_t)h->max_channels * (size_t)h->max_frames));
    *out = h;
    return PV_OK;
}

int pv_contour_set_stream(pv_contour *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_contour_set_stream: hipStreamSynchronize failed");
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_contour_synchronize(pv_contour *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_contour_synchronize: hipStreamSynchronize failed");
    return PV_OK;
}

int pv_contour_track_device(pv_contour *h, const float *d_in, int32_t nch, int64_t nframes, int64_t in_stride, int32_t bias, int32_t *d_candidates,
                            int64_t cand_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check(h, "pv_contour_track_device", d_in, d_candidates, nch, nframes, in_stride, bias, cand_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    if (((uintptr_t)d_candidates & 15) != 0)
        return fail(h, PV_ERR_ARGUMENT, "pv_contour_track_device: candidates must be 16-byte aligned (one store per slot)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, pv_launch_contour(d_in, (long)in_stride, nch, (int)nframes, h->W, h->hop, h->min_lag, h->max_lag, h->K, bias, d_candidates, (long)cand_stride,
                                h->stream));
    return PV_OK;
}

int pv_contour_track(pv_contour *h, const float *in, int32_t nch, int64_t nframes, int64_t in_stride, int32_t bias, int32_t *candidates, int64_t cand_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check(h, "pv_contour_track", in, candidates, nch, nframes, in_stride, bias, cand_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t piece_span = span(h, h->max_frames);
    const size_t fbytes = 16 * (size_t)h->K;                             // one frame's table
    for (int64_t m0 = 0; m0 < nframes; m0 += h->max_frames) {           // pieces of max_frames frames; a piece re-reads the W + max_lag - hop samples it shares
        const int64_t F = nframes - m0 < h->max_frames ? nframes - m0 : h->max_frames;
        const size_t row = sizeof(float) * (size_t)span(h, F);
        HIPCHK(h, hipMemcpy2DAsync(h->d_in, sizeof(float) * (size_t)piece_span, in + m0 * h->hop, sizeof(float) * (size_t)(nch > 1 ? in_stride : span(h, F)), row,
                                   nch, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, pv_launch_contour(h->d_in, (long)piece_span, nch, (int)F, h->W, h->hop, h->min_lag, h->max_lag, h->K, bias, h->d_cand, h->max_frames, h->stream));
        HIPCHK(h, hipMemcpy2DAsync(candidates + 4 * (int64_t)h->K * m0, fbytes * (size_t)(nch > 1 ? cand_stride : F), h->d_cand, fbytes * (size_t)h->max_frames,
                                   fbytes * (size_t)F, nch, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PV_OK;
}

}  // extern "C"
