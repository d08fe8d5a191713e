// pv_pitch_capi.hip -- the pv_pitch_* entry points of include/phaze_amd.h: pitch shifting through the time stretch.
//
// A pv_pitch owns one pv_stretch and one pv_resample and drives them through their PUBLIC device forms only (pv_transient_process_device, then
// pv_resample_process_device, on one stream): the stretch changes the duration by hs / ha at constant pitch, the resampler at up / down changes
// duration and pitch together, and with up / down = ha / hs the duration is back where it started while the pitch has moved by hs / ha.  The
// intermediate signal lives in a device buffer of the handle and never visits the host.  There is no kernel of its own here.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../host/pv_host_common.h"

struct pv_pitch {
    uint32_t magic;
    int N, ha, hs, max_channels, device;
    pv_stretch *stretch;
    pv_resample *resample;
    hipStream_t own_stream, stream;
    float *d_mid, *d_in, *d_out;             // the stretched signal; host-pointer calls: the input and output, all grown on demand
    size_t mid_cap, in_cap, out_cap;         // (in floats)
    char err[384];
};

namespace {

PV_HOST_HANDLE(pv_pitch, 0x50565054u /* 'PVPT' */, pv_pitch_destroy);

// Device pointers, asynchronous on h->stream.  The stretch validates its own arguments (and rejects with its state untouched) before the resampler moves.
int run(pv_pitch *h, const char *fn, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
        const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride, int64_t out_capacity, int64_t *nout)
{
    if (nch < 0 || nframes < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel or frame count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    const int64_t mid = (int64_t)nframes * h->hs;
    int64_t total = 0;
    (void)pv_resample_out_count(h->resample, mid, &total);
    if (nout) *nout = total;
    if (out_capacity < total)
        return failf(h, PV_ERR_ARGUMENT, "%s: out_capacity %lld is below the %lld samples per channel this call produces", fn, (long long)out_capacity,
                     (long long)total);
    if (nch > 1 && out_stride < total) return failf(h, PV_ERR_ARGUMENT, "%s: out_stride shorter than the samples produced (%lld)", fn, (long long)total);
    if (total > 0 && !d_out) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch == 0 || nframes == 0) return PV_OK;
    int rc = grow(h, &h->d_mid, &h->mid_cap, (size_t)nch * (size_t)mid);
    if (rc != PV_OK) return rc;
    rc = pv_transient_process_device(h->stretch, d_in, h->d_mid, nch, nframes, hops, hop_stride, resets, reset_stride, in_stride, mid);
    if (rc != PV_OK) return failf(h, rc, "%s: %s", fn, pv_stretch_last_error(h->stretch));
    rc = pv_resample_process_device(h->resample, h->d_mid, nch, mid, mid, d_out, out_stride, out_capacity, nullptr);
    if (rc != PV_OK) return failf(h, rc, "%s: %s", fn, pv_resample_last_error(h->resample));
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_pitch_last_error(const pv_pitch *h) { return last_error(h); }

int pv_pitch_destroy(pv_pitch *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stretch) (void)pv_stretch_destroy(h->stretch);
    if (h->resample) (void)pv_resample_destroy(h->resample);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    void *ptrs[] = {h->d_mid, h->d_in, h->d_out};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    (void)hipGetLastError();
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_pitch_create(const pv_pitch_config *cfg, pv_pitch **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_pitch_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_pitch_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_pitch_create: pv_pitch_config.struct_size does not match this library (start from PV_PITCH_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_pitch_create: unknown bits in pv_pitch_config.flags (must be 0)");
    int32_t up = cfg->up, down = cfg->down;
    if (up == 0 && down == 0) { up = cfg->analysis_hop; down = cfg->synthesis_hop; }     // constant duration: pitch x hs / ha
    if (pv_resample_count(up, down, 0) < 0)
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_pitch_create: up / down (0 / 0: analysis_hop / synthesis_hop) must be positive, within [1/8, 8], terms <= 8192 once reduced");

    pv_stretch_config sc = PV_STRETCH_CONFIG_INIT;
    sc.fft_size = cfg->fft_size; sc.analysis_hop = cfg->analysis_hop; sc.synthesis_hop = cfg->synthesis_hop;
    sc.max_channels = cfg->max_channels; sc.max_frames = 1; sc.device_id = cfg->device_id;
    pv_stretch *st = nullptr;
    int rc = pv_stretch_create(&sc, &st);
    if (rc != PV_OK) return fail(kNoHandle, rc, pv_stretch_last_error(nullptr));
    pv_resample_config rcfg = PV_RESAMPLE_CONFIG_INIT;
    rcfg.up = up; rcfg.down = down; rcfg.max_channels = cfg->max_channels; rcfg.max_samples = 1; rcfg.device_id = cfg->device_id;
    pv_resample *rs = nullptr;
    rc = pv_resample_create(&rcfg, &rs);
    if (rc != PV_OK) { (void)pv_stretch_destroy(st); return fail(kNoHandle, rc, pv_resample_last_error(nullptr)); }

    pv_pitch *h = (pv_pitch *)calloc(1, sizeof(pv_pitch));
    if (!h) { (void)pv_stretch_destroy(st); (void)pv_resample_destroy(rs); return fail(kNoHandle, PV_ERR_DEVICE, "pv_pitch_create: out of host memory"); }
    h->magic = HostTraits<pv_pitch>::kMagic;
    h->N = cfg->fft_size; h->ha = cfg->analysis_hop; h->hs = cfg->synthesis_hop;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    h->device = cfg->device_id;
    h->stretch = st; h->resample = rs;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        const size_t words = (size_t)h->max_channels * (size_t)(cfg->max_frames > 0 ? cfg->max_frames : 1) * (size_t)h->hs;
        e = hipMalloc(&h->d_mid, words * sizeof(float));
        if (e == hipSuccess) h->mid_cap = words;
    }
    if (e != hipSuccess) { (void)pv_pitch_destroy(h); return failf(kNoHandle, PV_ERR_DEVICE, "pv_pitch_create: %s", hipGetErrorString(e)); }
    rc = pv_pitch_set_stream(h, nullptr);
    if (rc != PV_OK) { fail(kNoHandle, rc, h->err); (void)pv_pitch_destroy(h); return rc; }
    *out = h;
    return PV_OK;
}

int pv_pitch_reset(pv_pitch *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    int rc = pv_stretch_reset(h->stretch);
    if (rc != PV_OK) return fail(h, rc, pv_stretch_last_error(h->stretch));
    rc = pv_resample_reset(h->resample);
    if (rc != PV_OK) return fail(h, rc, pv_resample_last_error(h->resample));
    return PV_OK;
}

// Both inner handles run on ONE stream: the caller's, or the pitch handle's own
int pv_pitch_set_stream(pv_pitch *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    if (h->stream && hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_pitch_set_stream: hipStreamSynchronize failed");
    int rc = pv_stretch_set_stream(h->stretch, s);
    if (rc != PV_OK) return fail(h, rc, pv_stretch_last_error(h->stretch));
    rc = pv_resample_set_stream(h->resample, s);
    if (rc != PV_OK) return fail(h, rc, pv_resample_last_error(h->resample));
    h->stream = s;
    return PV_OK;
}

int pv_pitch_synchronize(pv_pitch *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_pitch_synchronize: hipStreamSynchronize failed");
    return PV_OK;
}

pv_stretch *pv_pitch_stretch(pv_pitch *h) { return live(h) ? h->stretch : nullptr; }
pv_resample *pv_pitch_resampler(pv_pitch *h) { return live(h) ? h->resample : nullptr; }

int pv_pitch_process_device(pv_pitch *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
                            const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride, int64_t out_capacity, int64_t *nout)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_pitch_process_device: hipSetDevice failed");
    return run(h, "pv_pitch_process_device", d_in, d_out, nch, nframes, hops, hop_stride, resets, reset_stride, in_stride, out_stride, out_capacity, nout);
}

int pv_pitch_process(pv_pitch *h, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride, const uint8_t *resets,
                     int64_t reset_stride, int64_t in_stride, int64_t out_stride, int64_t out_capacity, int64_t *nout)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (nch < 0 || nframes < 0) return fail(h, PV_ERR_ARGUMENT, "pv_pitch_process: negative channel or frame count");
    if (nch > h->max_channels) return fail(h, PV_ERR_CAPACITY, "pv_pitch_process: more channels than max_channels");
    if (hops && hop_stride != 0 && hop_stride < nframes) return fail(h, PV_ERR_ARGUMENT, "pv_pitch_process: hop_stride is neither 0 nor >= nframes");
    // the input each channel brings: its schedule row's total (the stretch checks the hops themselves; here they only must not overflow the sum)
    int64_t most = (int64_t)nframes * h->ha;
    if (hops) {
        most = 0;
        for (int r = 0; r < (hop_stride == 0 ? 1 : nch); r++) {
            int64_t t = 0;
            for (int m = 0; m < nframes; m++) {
                const int32_t v = hops[(size_t)r * (size_t)hop_stride + m];
                if (v < 1 || v > h->N)
                    return failf(h, PV_ERR_ARGUMENT, "pv_pitch_process: hop %d of channel %d, frame %d is outside [1, fft_size %d]", (int)v, r, m, h->N);
                t += v;
            }
            if (t > most) most = t;
        }
    }
    int64_t total = 0;
    (void)pv_resample_out_count(h->resample, (int64_t)nframes * h->hs, &total);
    if (nout) *nout = total;
    if (out_capacity < total)
        return failf(h, PV_ERR_ARGUMENT, "pv_pitch_process: out_capacity %lld is below the %lld samples per channel this call produces", (long long)out_capacity,
                     (long long)total);
    if (!in || (total > 0 && !out)) return fail(h, PV_ERR_ARGUMENT, "pv_pitch_process: null buffer");
    if (nch > 1 && (in_stride < most || out_stride < total)) return fail(h, PV_ERR_ARGUMENT, "pv_pitch_process: channel strides shorter than the input read or the output written");
    if (nch == 0 || nframes == 0) return PV_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_pitch_process: hipSetDevice failed");
    const size_t dpitch_out = (size_t)(total > 0 ? total : 1);
    int rc = grow(h, &h->d_in, &h->in_cap, (size_t)nch * (size_t)most);
    if (rc == PV_OK) rc = grow(h, &h->d_out, &h->out_cap, (size_t)nch * dpitch_out);
    if (rc != PV_OK) return rc;
    hipError_t e = hipMemcpy2DAsync(h->d_in, sizeof(float) * (size_t)most, in, sizeof(float) * (size_t)(nch > 1 ? in_stride : most), sizeof(float) * (size_t)most,
                                    nch, hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_pitch_process: copy to the device failed");
    rc = run(h, "pv_pitch_process", h->d_in, h->d_out, nch, nframes, hops, hop_stride, resets, reset_stride, most, (int64_t)dpitch_out, (int64_t)dpitch_out, nullptr);
    if (rc != PV_OK) return rc;
    if (total > 0)
        e = hipMemcpy2DAsync(out, sizeof(float) * (size_t)(nch > 1 ? out_stride : total), h->d_out, sizeof(float) * dpitch_out, sizeof(float) * (size_t)total, nch,
                             hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_pitch_process: copy from the device failed");
    return PV_OK;
}

}  // extern "C"
