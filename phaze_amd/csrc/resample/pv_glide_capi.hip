// pv_glide_capi.hip -- the pv_glide_* entry points of include/phaze_amd.h: pitch curves through the time stretch.
//
// A pv_glide owns one pv_stretch (analysis_hop = min_hop, the floor of every schedule) and one pv_vari (block = synthesis_hop, counts within
// [min_hop, max_hop]) and drives them through their PUBLIC device forms only (pv_transient_process_device, then pv_vari_process_device, on one
// stream) with ONE row of hops: frame m consumes hops[m] input samples and the stretch emits hs for it, which the resampler turns back into hops[m]
// samples.  Duration is kept sample for sample, frame m is shifted in pitch by hs / hops[m].  The stretched signal lives in a device buffer of
// the handle and never visits the host.  There is no kernel of its own here.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../host/pv_host_common.h"

struct pv_glide {
    uint32_t magic;
    int N, hs, min_hop, max_hop, max_channels, device;
    pv_stretch *stretch;
    pv_vari *vari;
    hipStream_t own_stream, stream;
    float *d_mid, *d_in, *d_out;             // the stretched signal; host-pointer calls: the input and output, all grown on demand
    size_t mid_cap, in_cap, out_cap;         // (in floats)
    char err[384];
};

namespace {

PV_HOST_HANDLE(pv_glide, 0x5056474cu /* 'PVGL' */, pv_glide_destroy);

// What both forms check before any device work (the stretch adds its own: reset flags and rows, linked groups).  *total = the sum of the hops.
int check(pv_glide *h, const char *fn, const void *in, const void *out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t in_stride, int64_t out_stride,
          int64_t *total)
{
    if (nch < 0 || nframes < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel or frame count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (nframes > 0 && !hops) return failf(h, PV_ERR_ARGUMENT, "%s: null hops", fn);
    int64_t sum = 0;
    for (int m = 0; m < nframes; m++) {
        if (hops[m] < h->min_hop || hops[m] > h->max_hop)
            return failf(h, PV_ERR_ARGUMENT, "%s: hop %d of frame %d is outside [min_hop %d, max_hop %d]", fn, (int)hops[m], m, h->min_hop, h->max_hop);
        sum += hops[m];
    }
    *total = sum;
    if (sum > 0 && (!in || !out)) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch > 1 && (in_stride < sum || out_stride < sum))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the %lld samples per channel read and written", fn, (long long)sum);
    return PV_OK;
}

// Device pointers, asynchronous on h->stream.  The stretch validates the rest (and rejects with its state untouched) before the resampler moves;
// everything the resampler could reject has been checked by then.
int run(pv_glide *h, const char *fn, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops, const uint8_t *resets,
        int64_t reset_stride, int64_t in_stride, int64_t out_stride, int64_t total)
{
    const int64_t mid = (int64_t)nframes * h->hs;
    int rc = grow(h, &h->d_mid, &h->mid_cap, (size_t)nch * (size_t)mid);
    if (rc != PV_OK) return rc;
    rc = pv_transient_process_device(h->stretch, d_in, h->d_mid, nch, nframes, hops, 0, resets, reset_stride, in_stride, mid);
    if (rc != PV_OK) return failf(h, rc, "%s: %s", fn, pv_stretch_last_error(h->stretch));
    rc = pv_vari_process_device(h->vari, h->d_mid, nch, nframes, hops, mid, d_out, out_stride, total, nullptr);
    if (rc != PV_OK) return failf(h, rc, "%s: %s", fn, pv_vari_last_error(h->vari));
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_glide_last_error(const pv_glide *h) { return last_error(h); }

int pv_glide_destroy(pv_glide *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stretch) (void)pv_stretch_destroy(h->stretch);
    if (h->vari) (void)pv_vari_destroy(h->vari);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    void *ptrs[] = {h->d_mid, h->d_in, h->d_out};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    (void)hipGetLastError();
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_glide_create(const pv_glide_config *cfg, pv_glide **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_glide_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_glide_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_glide_create: pv_glide_config.struct_size does not match this library (start from PV_GLIDE_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_glide_create: unknown bits in pv_glide_config.flags (must be 0)");
    // the resampler's config errors, then the one of the pair, then the stretch's: all of them before any device is touched
    if (pv_vari_half_width(cfg->synthesis_hop, cfg->min_hop, cfg->max_hop) < 0)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_glide_create: %s (block = synthesis_hop, counts = hops)", pv_vari_last_error(nullptr));
    if (cfg->max_hop > cfg->fft_size && cfg->fft_size > 0)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_glide_create: max_hop %d is above fft_size %d (a frame's hop cannot exceed its window)", (int)cfg->max_hop,
                     (int)cfg->fft_size);

    pv_stretch_config sc = PV_STRETCH_CONFIG_INIT;
    sc.fft_size = cfg->fft_size; sc.analysis_hop = cfg->min_hop; sc.synthesis_hop = cfg->synthesis_hop;
    sc.max_channels = cfg->max_channels; sc.max_frames = 1; sc.device_id = cfg->device_id;
    pv_stretch *st = nullptr;
    int rc = pv_stretch_create(&sc, &st);
    if (rc != PV_OK) return fail(kNoHandle, rc, pv_stretch_last_error(nullptr));
    pv_vari_config vc = PV_VARI_CONFIG_INIT;
    vc.block = cfg->synthesis_hop; vc.min_count = cfg->min_hop; vc.max_count = cfg->max_hop;
    vc.max_channels = cfg->max_channels; vc.max_blocks = 1; vc.device_id = cfg->device_id;
    pv_vari *vr = nullptr;
    rc = pv_vari_create(&vc, &vr);
    if (rc != PV_OK) { (void)pv_stretch_destroy(st); return fail(kNoHandle, rc, pv_vari_last_error(nullptr)); }

    pv_glide *h = (pv_glide *)calloc(1, sizeof(pv_glide));
    if (!h) { (void)pv_stretch_destroy(st); (void)pv_vari_destroy(vr); return fail(kNoHandle, PV_ERR_DEVICE, "pv_glide_create: out of host memory"); }
    h->magic = HostTraits<pv_glide>::kMagic;
    h->N = cfg->fft_size; h->hs = cfg->synthesis_hop; h->min_hop = cfg->min_hop; h->max_hop = cfg->max_hop;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    h->device = cfg->device_id;
    h->stretch = st; h->vari = vr;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        const size_t words = (size_t)h->max_channels * (size_t)(cfg->max_frames > 0 ? cfg->max_frames : 1) * (size_t)h->hs;
        e = hipMalloc(&h->d_mid, words * sizeof(float));
        if (e == hipSuccess) h->mid_cap = words;
    }
    if (e != hipSuccess) { (void)pv_glide_destroy(h); return failf(kNoHandle, PV_ERR_DEVICE, "pv_glide_create: %s", hipGetErrorString(e)); }
    rc = pv_glide_set_stream(h, nullptr);
    if (rc != PV_OK) { fail(kNoHandle, rc, h->err); (void)pv_glide_destroy(h); return rc; }
    *out = h;
    return PV_OK;
}

int pv_glide_reset(pv_glide *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    int rc = pv_stretch_reset(h->stretch);
    if (rc != PV_OK) return fail(h, rc, pv_stretch_last_error(h->stretch));
    rc = pv_vari_reset(h->vari);
    if (rc != PV_OK) return fail(h, rc, pv_vari_last_error(h->vari));
    return PV_OK;
}

// Both inner handles run on ONE stream: the caller's, or the glide handle's own
int pv_glide_set_stream(pv_glide *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    if (h->stream && hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_glide_set_stream: hipStreamSynchronize failed");
    int rc = pv_stretch_set_stream(h->stretch, s);
    if (rc != PV_OK) return fail(h, rc, pv_stretch_last_error(h->stretch));
    rc = pv_vari_set_stream(h->vari, s);
    if (rc != PV_OK) return fail(h, rc, pv_vari_last_error(h->vari));
    h->stream = s;
    return PV_OK;
}

int pv_glide_synchronize(pv_glide *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_glide_synchronize: hipStreamSynchronize failed");
    return PV_OK;
}

pv_stretch *pv_glide_stretch(pv_glide *h) { return live(h) ? h->stretch : nullptr; }
pv_vari *pv_glide_resampler(pv_glide *h) { return live(h) ? h->vari : nullptr; }

int pv_glide_process_device(pv_glide *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops, const uint8_t *resets,
                            int64_t reset_stride, int64_t in_stride, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    int64_t total = 0;
    const int rc = check(h, "pv_glide_process_device", d_in, d_out, nch, nframes, hops, in_stride, out_stride, &total);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_glide_process_device: hipSetDevice failed");
    return run(h, "pv_glide_process_device", d_in, d_out, nch, nframes, hops, resets, reset_stride, in_stride, out_stride, total);
}

int pv_glide_process(pv_glide *h, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops, const uint8_t *resets, int64_t reset_stride,
                     int64_t in_stride, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    int64_t total = 0;
    int rc = check(h, "pv_glide_process", in, out, nch, nframes, hops, in_stride, out_stride, &total);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_glide_process: hipSetDevice failed");
    rc = grow(h, &h->d_in, &h->in_cap, (size_t)nch * (size_t)total);
    if (rc == PV_OK) rc = grow(h, &h->d_out, &h->out_cap, (size_t)nch * (size_t)total);
    if (rc != PV_OK) return rc;
    const size_t row = sizeof(float) * (size_t)total;
    hipError_t e = hipMemcpy2DAsync(h->d_in, row, in, sizeof(float) * (size_t)(nch > 1 ? in_stride : total), row, nch, hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_glide_process: copy to the device failed");
    rc = run(h, "pv_glide_process", h->d_in, h->d_out, nch, nframes, hops, resets, reset_stride, total, total, total);
    if (rc != PV_OK) return rc;
    e = hipMemcpy2DAsync(out, sizeof(float) * (size_t)(nch > 1 ? out_stride : total), h->d_out, row, row, nch, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, PV_ERR_DEVICE, "pv_glide_process: copy from the device failed");
    return PV_OK;
}

}  // extern "C"
