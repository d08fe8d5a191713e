// pv_epoch_capi.hip -- the pv_epoch_* handle entry points of include/phaze_amd.h: the epoch records (kernel: pv_epoch_kernels.hip), and
// pv_epoch_periods, the host code that turns f0 records into the period row the kernel reads.
//
// A pv_epoch holds a geometry (window, hop, longest period) and the staging buffers of the host-pointer form; it carries no state from call to
// call.  pv_epoch_plan, the planner that consumes the records, is in pv_epoch_plan.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../host/pv_host_common.h"
#include "pv_epoch.h"

struct pv_epoch {
    uint32_t magic;
    int W, hop, max_period, max_channels, max_frames, device;
    hipStream_t own_stream, stream;
    float *d_in;                             // host-pointer calls: one piece of input, [max_channels][(max_frames - 1) hop + W]
    int32_t *d_per;                          // its periods, [max_frames]
    int32_t *d_rec;                          // and its records, [max_channels][max_frames][4]
    char err[384];
};

namespace {

PV_HOST_HANDLE(pv_epoch, 0x50564550u /* 'PVEP' */, pv_epoch_destroy);

int64_t span(const pv_epoch *h, int64_t nframes) { return (nframes - 1) * h->hop + h->W; }

// What both forms check before any device work.
int check(pv_epoch *h, const char *fn, const void *in, const void *periods, const void *records, int32_t nch, int64_t nframes, int64_t in_stride,
          int64_t rec_stride)
{
    if (nch < 0 || nframes < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel or frame count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (nframes > 0x7fffffff) return failf(h, PV_ERR_ARGUMENT, "%s: more than 2^31 - 1 frames in one call", fn);
    if (nch == 0 || nframes == 0) return PV_OK;
    if (!in || !periods || !records) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch > 1 && (in_stride < span(h, nframes) || rec_stride < nframes))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the %lld samples read and the %lld records written per channel", fn,
                     (long long)span(h, nframes), (long long)nframes);
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_epoch_last_error(const pv_epoch *h) { return last_error(h); }

int pv_epoch_destroy(pv_epoch *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->d_in) (void)hipFree(h->d_in);
    if (h->d_per) (void)hipFree(h->d_per);
    if (h->d_rec) (void)hipFree(h->d_rec);
    (void)hipGetLastError();
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_epoch_create(const pv_epoch_config *cfg, pv_epoch **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_epoch_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_epoch_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_epoch_create: pv_epoch_config.struct_size does not match this library (start from PV_EPOCH_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_epoch_create: unknown bits in pv_epoch_config.flags (must be 0)");
    if (cfg->max_period < PV_EPOCH_MIN_PERIOD || cfg->max_period > PV_EPOCH_MAX_PERIOD)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_epoch_create: max_period %d is outside [%d, %d]", (int)cfg->max_period, PV_EPOCH_MIN_PERIOD, PV_EPOCH_MAX_PERIOD);
    if (cfg->window < 2 * cfg->max_period || cfg->window > PV_EPOCH_MAX_WINDOW)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_epoch_create: window %d is outside [2 max_period, %d]", (int)cfg->window, PV_EPOCH_MAX_WINDOW);
    if (cfg->hop < 1 || cfg->hop > PV_EPOCH_MAX_HOP)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_epoch_create: hop %d is outside [1, %d]", (int)cfg->hop, PV_EPOCH_MAX_HOP);
    if (cfg->max_channels < 0 || cfg->max_channels > 65535)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_epoch_create: max_channels %d is outside [0, 65535]", (int)cfg->max_channels);
    if (cfg->max_frames < 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_epoch_create: negative max_frames");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_epoch *h = (pv_epoch *)calloc(1, sizeof(pv_epoch));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_epoch_create: out of host memory");
    h->magic = HostTraits<pv_epoch>::kMagic;
    h->W = cfg->window; h->hop = cfg->hop; h->max_period = cfg->max_period;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    h->max_frames = cfg->max_frames > 0 ? cfg->max_frames : 256;
    h->device = cfg->device_id;
    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    CREATE_CHK(h, hipMalloc(&h->d_in, sizeof(float) * (size_t)h->max_channels * (size_t)span(h, h->max_frames)));
    CREATE_CHK(h, hipMalloc(&h->d_per, sizeof(int32_t) * (size_t)h->max_frames));
    CREATE_CHK(h, hipMalloc(&h->d_rec, sizeof(int32_t) * 4 * (size_t)h->max_channels * (size_t)h->max_frames));
    *out = h;
    return PV_OK;
}

int pv_epoch_set_stream(pv_epoch *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_epoch_set_stream: hipStreamSynchronize failed");
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_epoch_synchronize(pv_epoch *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_epoch_synchronize: hipStreamSynchronize failed");
    return PV_OK;
}

int pv_epoch_track_device(pv_epoch *h, const float *d_in, int32_t nch, int64_t nframes, int64_t in_stride, const int32_t *d_periods256, int32_t *d_records,
                          int64_t rec_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check(h, "pv_epoch_track_device", d_in, d_periods256, d_records, nch, nframes, in_stride, rec_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    if (((uintptr_t)d_records & 15) != 0) return fail(h, PV_ERR_ARGUMENT, "pv_epoch_track_device: records must be 16-byte aligned (one store per record)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, pv_launch_epoch(d_in, (long)in_stride, nch, (int)nframes, h->W, h->hop, h->max_period, d_periods256, d_records, (long)rec_stride, h->stream));
    return PV_OK;
}

int pv_epoch_track(pv_epoch *h, const float *in, int32_t nch, int64_t nframes, int64_t in_stride, const int32_t *periods256, int32_t *records, int64_t rec_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check(h, "pv_epoch_track", in, periods256, records, nch, nframes, in_stride, rec_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t piece_span = span(h, h->max_frames);
    for (int64_t m0 = 0; m0 < nframes; m0 += h->max_frames) {           // pieces of max_frames frames; a piece re-reads the W - hop samples it shares
        const int64_t F = nframes - m0 < h->max_frames ? nframes - m0 : h->max_frames;
        const size_t row = sizeof(float) * (size_t)span(h, F);
        HIPCHK(h, hipMemcpy2DAsync(h->d_in, sizeof(float) * (size_t)piece_span, in + m0 * h->hop, sizeof(float) * (size_t)(nch > 1 ? in_stride : span(h, F)), row,
                                   nch, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_per, periods256 + m0, sizeof(int32_t) * (size_t)F, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, pv_launch_epoch(h->d_in, (long)piece_span, nch, (int)F, h->W, h->hop, h->max_period, h->d_per, h->d_rec, h->max_frames, h->stream));
        const size_t rrow = 16 * (size_t)F;
        HIPCHK(h, hipMemcpy2DAsync(records + 4 * m0, 16 * (size_t)(nch > 1 ? rec_stride : F), h->d_rec, 16 * (size_t)h->max_frames, rrow, nch, hipMemcpyDeviceToHost,
                                   h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PV_OK;
}

int64_t pv_epoch_periods(const int32_t *records, int64_t nrec, int32_t *periods256, int64_t capacity)
{
    if (nrec < 0 || (nrec > 0 && !records) || capacity < 0 || (capacity > 0 && !periods256)) return -PV_ERR_ARGUMENT;
    for (int64_t j = 0; j < nrec && j < capacity; j++) {
        const double v = floor(256.0 * pv_f0_period(records + 4 * j) + 0.5);                   // 0 where it is unvoiced
        periods256[j] = v < 2147483647.0 ? (v > -2147483648.0 ? (int32_t)v : INT32_MIN) : INT32_MAX;       // records that no tracker wrote: out of range either way
    }
    return nrec;
}

}  // extern "C"
