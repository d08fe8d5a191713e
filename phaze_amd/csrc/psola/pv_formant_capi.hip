// pv_formant_capi.hip -- host side of the pv_formant_* handle entry points of include/phaze_amd.h (overlap-add of grains that read the input at a step of their own).
//
// pv_tsm_capi.hip's shape: a pv_formant holds the two tables of the kernel (the prototype P of the variable-ratio resampler and the window table Hn), the
// staging buffers of the host-pointer form and the page-locked buffer a call's tables go through; it carries no signal state from call to call.  Per
// call the host validates every grain (pv_formant.h), then works out per tile of the output range the contiguous range of grains that can overlap the
// tile and the source range those grains read inside the tile, at their steps (pv_formant.h), refuses the call if a tile's range exceeds the
// handle's span, and uploads the grain table and one int4 per tile on the handle's stream.  pv_formant_plan is in pv_formant_plan.hip.
// No CPU compute path: without a HIP device pv_formant_create fails with PV_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "../host/pv_host_common.h"
#include "pv_formant.h"

namespace {
constexpr long long kMaxGrains = 1LL << 27;            // bounds the uploaded table (2 GiB of records)
constexpr int kDefaultOutputs = 1 << 16, kMaxOutputs = 1 << 24;
}  // namespace

struct pv_formant {
    uint32_t magic;
    int max_period, max_rate, max_channels, max_outputs, device;       // max_outputs: a multiple of the tile
    int span;                    // the longest source range a tile may have
    hipStream_t own_stream, stream;
    float *d_ptable, *d_htable;
    int *h_tab, *d_tab;          // the call's tables: grains[ngrains][4], then {g_first, g_end, src0, src_count} per tile
    size_t htab_cap, tab_cap;    // (in ints)
    hipEvent_t tab_done;
    bool tab_pending;
    float *d_stage_in, *d_stage_out;
    long long stage_in_pitch;
    std::vector<int64_t> *walk;  // the tile walk's int64 records
    char err[256];
};

namespace {

PV_HOST_HANDLE(pv_formant, 0x5056464Du /* 'PVFM' */, pv_formant_destroy);

// What both forms check before any device work.
int check_process(pv_formant *h, const char *fn, const void *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, const void *out,
                  int64_t out_first, int64_t nout, int64_t out_stride)
{
    if (nch < 0 || nin < 0 || ngrains < 0 || nout < 0 || out_first < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel, sample, grain or output count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (nin > PV_TSM_MAX_POSITION || out_first > PV_TSM_MAX_POSITION || nout > PV_TSM_MAX_POSITION || out_first + nout > PV_TSM_MAX_POSITION)
        return failf(h, PV_ERR_ARGUMENT, "%s: positions must stay below 2^30", fn);
    if (ngrains > kMaxGrains) return failf(h, PV_ERR_ARGUMENT, "%s: more than 2^27 grains in one call", fn);
    if ((ngrains > 0 && !grains) || (nch > 0 && nin > 0 && !in) || (nch > 0 && nout > 0 && !out)) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch > 1 && (in_stride < nin || out_stride < nout))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the input (%lld) or the outputs (%lld)", fn, (long long)nin, (long long)nout);
    int why = 0;
    const int64_t g = pv_formant_check_grains(grains, ngrains, h->max_period, &why);
    if (g < 0) return PV_OK;
    const int32_t t = grains[4 * g], w = grains[4 * g + 1], D = grains[4 * g + 2], L = grains[4 * g + 3];
    switch (why) {
    case PV_FORMANT_BAD_CENTRE:
        return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: centre %d is outside [0, 2^30)", fn, (long long)g, (int)t);
    case PV_FORMANT_BAD_STEP:
        return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: w = %d is outside [0, 2^27), has bit 16 set (no mirrored grains here) or a step %d that is neither 0 nor "
                     "within [128, 512]", fn, (long long)g, (int)w, (int)((w >> PV_FORMANT_STEP_SHIFT) & 1023));
    case PV_FORMANT_BAD_LENGTH:
        return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: half length %d is outside [2, max_period %d]", fn, (long long)g, (int)L, h->max_period);
    case PV_FORMANT_BAD_SHIFT:
        return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: displacement %d is not inside +-2^30", fn, (long long)g, (int)D);
    default:
        return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: its centre lies before the centre of grain %lld (out of order)", fn, (long long)g, (long long)g - 1);
    }
}

// The call's tables in the page-locked buffer: the grains, then per tile of [out_first, out_first + nout) the grain range and the source range.  Pure host
// work (the previous upload of the buffer is waited for first); refuses the call when a tile's source range exceeds the span.  *longest: the longest
// source range among the tiles.
int make_tables(pv_formant *h, const char *fn, const int32_t *grains, long long ngrains, long long out_first, long long nout, int *longest)
{
    const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE;
    const size_t gw = 4 * (size_t)(ngrains > 0 ? ngrains : 1), words = gw + 4 * (size_t)ntiles;
    h->walk->resize(4 * (size_t)ntiles);
    int64_t *walk = h->walk->data();
    pv_formant_tiles(grains, ngrains, h->max_period, out_first, nout, walk);
    *longest = 0;
    for (long long t = 0; t < ntiles; t++) {
        const long long extent = walk[4 * t + 3];
        if (extent > h->span) {
            const long long j0 = out_first + t * PV_TSM_TILE, j1 = j0 + (nout - t * PV_TSM_TILE < PV_TSM_TILE ? nout - t * PV_TSM_TILE : PV_TSM_TILE);
            return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: the tile of outputs [%lld, %lld) that begins with it reads %lld input samples, more than the span %d of "
                         "max_period %d and max_rate %d", fn, (long long)walk[4 * t], j0, j1, extent, h->span, h->max_period, h->max_rate);
        }
        if (extent > *longest) *longest = (int)extent;
    }
    // the page-locked table is rewritten only once the previous upload has completed, so a device call may follow another before any synchronise
    if (h->tab_pending) HIPCHK(h, hipEventSynchronize(h->tab_done));
    h->tab_pending = false;
    if (words > h->htab_cap) {
        if (h->h_tab) (void)hipHostFree(h->h_tab);
        h->h_tab = nullptr; h->htab_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->h_tab, words * sizeof(int), hipHostMallocDefault));
        h->htab_cap = words;
    }
    int *tiles = h->h_tab + gw;
    for (long long t = 0; t < ntiles; t++) {
        tiles[4 * t] = (int)walk[4 * t];
        tiles[4 * t + 1] = (int)walk[4 * t + 1];
        tiles[4 * t + 2] = pv_formant_src0(walk[4 * t + 2]);
        tiles[4 * t + 3] = (int)walk[4 * t + 3];
    }
    memset(h->h_tab, 0, 4 * sizeof(int));
    if (ngrains > 0) memcpy(h->h_tab, grains, 4 * sizeof(int) * (size_t)ngrains);
    return PV_OK;
}

// Uploads what make_tables made.  Asynchronous on h->stream.
int upload_tables(pv_formant *h, long long ngrains, long long nout)
{
    const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE;
    const size_t words = 4 * (size_t)(ngrains > 0 ? ngrains : 1) + 4 * (size_t)ntiles;
    const int rc = grow(h, &h->d_tab, &h->tab_cap, words);
    if (rc != PV_OK) return rc;
    if (!h->tab_done) HIPCHK(h, hipEventCreateWithFlags(&h->tab_done, hipEventDisableTiming));
    HIPCHK(h, hipMemcpyAsync(h->d_tab, h->h_tab, words * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->tab_done, h->stream));
    h->tab_pending = true;
    return PV_OK;
}

// One launch: outputs [out_first, out_first + nout) of the call whose tables are uploaded; tile0 is the index of the launch's first tile in them, `longest`
// the longest source range of the call's tiles (the launch's LDS is sized by it: a multiple of 64 samples, at least two tap rows).
int launch(pv_formant *h, const float *d_in, long long in_first, long long in_count, long in_stride, int nch, long long ngrains, float *d_out, long long out_first,
           long long nout, long out_stride, long long tile0, int longest)
{
    PvTsmParams p;
    memset(&p, 0, sizeof p);
    p.in = d_in; p.out = d_out; p.in_stride = in_stride; p.out_stride = out_stride;
    p.ptable = h->d_ptable; p.htable = h->d_htable;
    p.grains = (const int4 *)h->d_tab;
    p.tiles = (const int4 *)(h->d_tab + 4 * (size_t)(ngrains > 0 ? ngrains : 1)) + tile0;
    p.in_first = in_first; p.in_count = in_count;
    p.out_first = (int)out_first; p.nout = (int)nout; p.nch = nch;
    int span = (longest + 63) & ~63;
    if (span > h->span) span = h->span;                                  // the largest pair of a rate fills the LDS to within 64 samples: no rounding past it
    if (span < 2 * PV_FORMANT_TAPS) span = 2 * PV_FORMANT_TAPS;
    p.span = span;
    HIPCHK(h, pv_launch_formant(p, h->stream));
    return PV_OK;
}

// check_process and make_tables for either form; nothing has touched the device when this refuses.
int prepare(pv_formant *h, const char *fn, const void *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, const void *out,
            int64_t out_first, int64_t nout, int64_t out_stride, int *longest, bool *nothing)
{
    const int rc = check_process(h, fn, in, nin, in_stride, nch, grains, ngrains, out, out_first, nout, out_stride);
    if (rc != PV_OK) return rc;
    *nothing = nch == 0 || nout == 0;
    if (*nothing) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int r = make_tables(h, fn, grains, ngrains, out_first, nout, longest);
    if (r != PV_OK) return r;
    return upload_tables(h, ngrains, nout);
}

}  // namespace

extern "C" {

const char *pv_formant_last_error(const pv_formant *h) { return last_error(h); }

int pv_formant_create(const pv_formant_config *cfg, pv_formant **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_formant_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_formant_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_formant_create: pv_formant_config.struct_size does not match this library (start from PV_FORMANT_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_formant_create: unknown bits in pv_formant_config.flags (must be 0)");
    if (cfg->max_period < 2 || cfg->max_period > PV_TSM_MAX_PERIOD)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_formant_create: max_period %d is outside [2, 4096]", (int)cfg->max_period);
    if (cfg->max_rate < 1 || cfg->max_rate > PV_TSM_MAX_RATE) return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_formant_create: max_rate %d is outside [1, 4]", (int)cfg->max_rate);
    if (cfg->max_channels < 0 || cfg->max_channels > 65535)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_formant_create: max_channels %d is outside [0, 65535]", (int)cfg->max_channels);
    if (cfg->max_outputs < 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_formant_create: negative max_outputs");
    const int span = pv_formant_span(cfg->max_period, cfg->max_rate);
    if (pv_tsm_lds_bytes(span) > PV_TSM_LDS_BYTES)
        return failf(kNoHandle, PV_ERR_UNSUPPORTED, "pv_formant_create: max_period %d at max_rate %d stages %d samples per tile: %lld bytes of LDS with the tables, more than the "
                     "%d of a compute unit", (int)cfg->max_period, (int)cfg->max_rate, span, (long long)pv_tsm_lds_bytes(span), PV_TSM_LDS_BYTES);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_formant *h = (pv_formant *)calloc(1, sizeof(pv_formant));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_formant_create: out of host memory");
    h->magic = HostTraits<pv_formant>::kMagic;
    h->max_period = cfg->max_period;
    h->max_rate = cfg->max_rate;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    int mo = cfg->max_outputs > 0 ? cfg->max_outputs : kDefaultOutputs;
    if (mo > kMaxOutputs) mo = kMaxOutputs;
    h->max_outputs = (mo + PV_TSM_TILE - 1) / PV_TSM_TILE * PV_TSM_TILE;
    h->device = cfg->device_id;
    h->span = span;
    // what a piece of max_outputs outputs reads when it runs at max_rate, and never less than one tile's span
    h->stage_in_pitch = (long long)h->max_rate * ((long long)h->max_outputs + 2 * h->max_period) + 6 * h->max_period + 192;
    h->walk = new (std::nothrow) std::vector<int64_t>();
    if (!h->walk) {
        pv_formant_destroy(h);
        return fail(kNoHandle, PV_ERR_DEVICE, "pv_formant_create: out of host memory");
    }

    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    {
        std::vector<float> P(PV_VARI_TABLE_WORDS, 0.0f), H(PV_TSM_WINDOW_WORDS, 0.0f);
        if (pv_vari_prototype(P.data(), PV_VARI_TABLE) != PV_VARI_TABLE || pv_psola_window(H.data(), PV_TSM_WINDOW) != PV_TSM_WINDOW) {
            pv_formant_destroy(h);
            return fail(kNoHandle, PV_ERR_DEVICE, "pv_formant_create: no prototype or window table");
        }
        CREATE_CHK(h, hipMalloc(&h->d_ptable, sizeof(float) * P.size()));
        CREATE_CHK(h, hipMemcpy(h->d_ptable, P.data(), sizeof(float) * P.size(), hipMemcpyHostToDevice));
        CREATE_CHK(h, hipMalloc(&h->d_htable, sizeof(float) * H.size()));
        CREATE_CHK(h, hipMemcpy(h->d_htable, H.data(), sizeof(float) * H.size(), hipMemcpyHostToDevice));
    }
    CREATE_CHK(h, hipMalloc(&h->d_stage_in, sizeof(float) * (size_t)h->max_channels * (size_t)h->stage_in_pitch));
    CREATE_CHK(h, hipMalloc(&h->d_stage_out, sizeof(float) * (size_t)h->max_channels * (size_t)h->max_outputs));
    *out = h;
    return PV_OK;
}

int pv_formant_destroy(pv_formant *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->tab_done) (void)hipEventDestroy(h->tab_done);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->h_tab) (void)hipHostFree(h->h_tab);
    void *ptrs[] = {h->d_ptable, h->d_htable, h->d_tab, h->d_stage_in, h->d_stage_out};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    (void)hipGetLastError();
    delete h->walk;
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_formant_set_stream(pv_formant *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // work queued on the old stream is ordered before the new one's
    h->tab_pending = false;
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_formant_synchronize(pv_formant *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int pv_formant_process_device(pv_formant *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *d_out,
                             int64_t out_first, int64_t nout, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    try {
        int longest = 0;
        bool nothing = false;
        const int rc = prepare(h, "pv_formant_process_device", d_in, nin, in_stride, nch, grains, ngrains, d_out, out_first, nout, out_stride, &longest, &nothing);
        if (rc != PV_OK || nothing) return rc;
        return launch(h, d_in, 0, nin, (long)in_stride, nch, ngrains, d_out, out_first, nout, (long)out_stride, 0, longest);
    } catch (...) {
        return fail(h, PV_ERR_DEVICE, "pv_formant_process_device: out of host memory");
    }
}

int pv_formant_process(pv_formant *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *out, int64_t out_first,
                      int64_t nout, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    try {
        int longest = 0;
        bool nothing = false;
        const int rc = prepare(h, "pv_formant_process", in, nin, in_stride, nch, grains, ngrains, out, out_first, nout, out_stride, &longest, &nothing);
        if (rc != PV_OK || nothing) return rc;
        // Pieces of whole tiles through the staging buffers, as pv_tsm_process: a piece stages the hull of its tiles' source ranges cut to the input.  It
        // takes as many tiles as fit max_outputs and whose hull fits the staging buffer, and always at least one: one tile's range is at most the span,
        // which the buffer holds.
        const int *tiles = h->h_tab + 4 * (size_t)(ngrains > 0 ? ngrains : 1);
        const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE, most = h->max_outputs / PV_TSM_TILE;
        const size_t ipitch = sizeof(float) * (size_t)(nch > 1 ? in_stride : (nin > 0 ? nin : 1)), opitch = sizeof(float) * (size_t)(nch > 1 ? out_stride : nout);
        for (long long t0 = 0; t0 < ntiles;) {
            long long a = 0, b = 0, t1 = t0;
            bool any = false;
            while (t1 < ntiles && t1 - t0 < most) {
                long long na = a, nb = b;
                bool nany = any;
                if (tiles[4 * t1 + 3] > 0) {
                    long long s0 = tiles[4 * t1 + 2], s1 = s0 + tiles[4 * t1 + 3];
                    if (s0 < 0) s0 = 0;
                    if (s1 > nin) s1 = nin;
                    if (s1 > s0) {
                        na = !any || s0 < a ? s0 : a;
                        nb = !any || s1 > b ? s1 : b;
                        nany = true;
                    }
                }
                if (t1 > t0 && nb - na > h->stage_in_pitch) break;
                a = na; b = nb; any = nany;
                t1++;
            }
            const long long at = t0 * PV_TSM_TILE, m = (t1 * PV_TSM_TILE < nout ? t1 * PV_TSM_TILE : nout) - at, o = out_first + at;
            if (b > a)
                HIPCHK(h, hipMemcpy2DAsync(h->d_stage_in, sizeof(float) * (size_t)h->stage_in_pitch, in + a, ipitch, sizeof(float) * (size_t)(b - a), nch, hipMemcpyHostToDevice,
                                           h->stream));
            const int lr = launch(h, h->d_stage_in, a, b - a, (long)h->stage_in_pitch, nch, ngrains, h->d_stage_out, o, m, (long)h->max_outputs, t0, longest);
            if (lr != PV_OK) return lr;
            HIPCHK(h, hipMemcpy2DAsync(out + at, opitch, h->d_stage_out, sizeof(float) * (size_t)h->max_outputs, sizeof(float) * (size_t)m, nch, hipMemcpyDeviceToHost,
                                       h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            t0 = t1;
        }
        return PV_OK;
    } catch (...) {
        return fail(h, PV_ERR_DEVICE, "pv_formant_process: out of host memory");
    }
}

}  // extern "C"
