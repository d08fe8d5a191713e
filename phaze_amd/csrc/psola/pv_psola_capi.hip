// pv_psola_capi.hip -- host side of the pv_psola_* entry points of include/phaze_amd.h (pitch-synchronous overlap-add).
//
// A pv_psola holds the two tables of the kernel (the prototype P of the variable-ratio resampler and the window table Hn), the staging buffers of the
// host-pointer form and the page-locked buffer a call's grain table goes through; it carries no signal state from call to call.  Per call the
// host validates every grain, then uploads the table and, per tile of the output range, the contiguous range of grains that can overlap the tile
// (a two-pointer walk over the centres, trimmed to the grains that reach the tile), on the handle's stream.  pv_psola_window is pure host code;
// pv_psola_plan and pv_psola_ratios are in pv_psola_plan.hip.
// No CPU compute path: without a HIP device pv_psola_create fails with PV_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../host/pv_host_common.h"
#include "pv_psola.h"

namespace {
constexpr long long kMaxGrains = 1LL << 27;            // bounds the uploaded table (2 GiB of records)
constexpr int kDefaultOutputs = 1 << 16, kMaxOutputs = 1 << 24;

// Hn[q] = f32((1 + cos(pi q / 1024)) / 2) for q < 1024; 0 from 1024 on
void window(float *H, size_t n)
{
    for (size_t q = 0; q < n; q++) H[q] = q < 1024 ? (float)(0.5 * (1.0 + cos(M_PI * (double)q / 1024.0))) : 0.0f;
}
}  // namespace

struct pv_psola {
    uint32_t magic;
    int max_period, max_channels, max_outputs, device;       // max_outputs: a multiple of the tile
    int span;
    hipStream_t own_stream, stream;
    float *d_ptable, *d_htable;
    int *h_tab, *d_tab;          // the call's tables: grains[ngrains][4], then [first, end) per tile
    size_t htab_cap, tab_cap;    // (in ints)
    hipEvent_t tab_done;
    bool tab_pending;
    float *d_stage_in, *d_stage_out;
    long long stage_in_pitch;
    char err[256];
};

namespace {

PV_HOST_HANDLE(pv_psola, 0x50565053u /* 'PVPS' */, pv_psola_destroy);

// What both forms check before any device work.
int check_process(pv_psola *h, const char *fn, const void *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, const void *out,
                  int64_t out_first, int64_t nout, int64_t out_stride)
{
    if (nch < 0 || nin < 0 || ngrains < 0 || nout < 0 || out_first < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel, sample, grain or output count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (nin > PV_PSOLA_MAX_POSITION || out_first > PV_PSOLA_MAX_POSITION || nout > PV_PSOLA_MAX_POSITION || out_first + nout > PV_PSOLA_MAX_POSITION)
        return failf(h, PV_ERR_ARGUMENT, "%s: positions must stay below 2^30", fn);
    if (ngrains > kMaxGrains) return failf(h, PV_ERR_ARGUMENT, "%s: more than 2^27 grains in one call", fn);
    if ((ngrains > 0 && !grains) || (nch > 0 && nin > 0 && !in) || (nch > 0 && nout > 0 && !out)) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch > 1 && (in_stride < nin || out_stride < nout))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the input (%lld) or the outputs (%lld)", fn, (long long)nin, (long long)nout);
    long long prev = 0;
    for (int64_t g = 0; g < ngrains; g++) {
        const int32_t t = grains[4 * g], tf = grains[4 * g + 1], dq = grains[4 * g + 2], L = grains[4 * g + 3];
        if (t < 0 || t >= PV_PSOLA_MAX_POSITION || tf < 0 || tf >= PV_PSOLA_Q)
            return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: centre %d + %d / 256 is outside [0, 2^30) or its fraction outside [0, 255]", fn, (long long)g, (int)t, (int)tf);
        if (L < 2 || L > h->max_period) return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: half length %d is outside [2, max_period %d]", fn, (long long)g, (int)L, h->max_period);
        if (dq < -PV_PSOLA_Q * h->max_period || dq > PV_PSOLA_Q * h->max_period)
            return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: shift %d is outside +-256 * max_period %d", fn, (long long)g, (int)dq, h->max_period);
        const long long c = (long long)t * PV_PSOLA_Q + tf;
        if (c < prev) return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: its centre lies before the centre of grain %lld (out of order)", fn, (long long)g, (long long)g - 1);
        prev = c;
    }
    return PV_OK;
}

// Uploads the call's grain table and the grain range of every tile of [out_first, out_first + nout).  Asynchronous on h->stream.
int upload_tables(pv_psola *h, const int32_t *grains, long long ngrains, long long out_first, long long nout)
{
    const long long ntiles = (nout + PV_PSOLA_TILE - 1) / PV_PSOLA_TILE;
    const size_t gw = 4 * (size_t)(ngrains > 0 ? ngrains : 1), words = gw + 2 * (size_t)ntiles;
    // the page-locked table is rewritten only once the previous upload has completed, so a device call may follow another before any synchronise
    if (h->tab_pending) HIPCHK(h, hipEventSynchronize(h->tab_done));
    h->tab_pending = false;
    if (words > h->htab_cap) {
        if (h->h_tab) (void)hipHostFree(h->h_tab);
        h->h_tab = nullptr; h->htab_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->h_tab, words * sizeof(int), hipHostMallocDefault));
        h->htab_cap = words;
    }
    const int rc = grow(h, &h->d_tab, &h->tab_cap, words);
    if (rc != PV_OK) return rc;
    if (!h->tab_done) HIPCHK(h, hipEventCreateWithFlags(&h->tab_done, hipEventDisableTiming));
    memset(h->h_tab, 0, 4 * sizeof(int));
    if (ngrains > 0) memcpy(h->h_tab, grains, 4 * sizeof(int) * (size_t)ngrains);
    int *tiles = h->h_tab + gw;
    const long long mp = h->max_period;
    long long lo = 0, hi = 0;
    for (long long t = 0; t < ntiles; t++) {
        const long long j0 = out_first + t * PV_PSOLA_TILE, j1 = j0 + (nout - t * PV_PSOLA_TILE < PV_PSOLA_TILE ? nout - t * PV_PSOLA_TILE : PV_PSOLA_TILE);
        // centres are in order and no half length is above max_period: a grain that reaches [j0, j1) has its centre t within [j0 - mp - 1, j1 + mp)
        while (lo < ngrains && grains[4 * lo] < j0 - mp - 1) lo++;
        if (hi < lo) hi = lo;
        while (hi < ngrains && grains[4 * hi] < j1 + mp) hi++;
        long long a = lo, b = hi;                                       // trimmed to the first and the last grain that reach the tile
        while (a < b && (long long)grains[4 * a] + 1 + grains[4 * a + 3] <= j0) a++;
        while (b > a && (long long)grains[4 * (b - 1)] - grains[4 * (b - 1) + 3] >= j1) b--;
        tiles[2 * t] = (int)a;
        tiles[2 * t + 1] = (int)b;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_tab, h->h_tab, words * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->tab_done, h->stream));
    h->tab_pending = true;
    return PV_OK;
}

// One launch: outputs [out_first, out_first + nout) of the call whose tables are uploaded; tile0 is the index of the launch's first tile in them.
int launch(pv_psola *h, const float *d_in, long long in_first, long long in_count, long in_stride, int nch, long long ngrains, float *d_out, long long out_first,
           long long nout, long out_stride, long long tile0)
{
    PvPsolaParams p;
    memset(&p, 0, sizeof p);
    p.in = d_in; p.out = d_out; p.in_stride = in_stride; p.out_stride = out_stride;
    p.ptable = h->d_ptable; p.htable = h->d_htable;
    p.grains = (const int4 *)h->d_tab;
    p.tile_grains = (const int2 *)(h->d_tab + 4 * (size_t)(ngrains > 0 ? ngrains : 1)) + tile0;
    p.in_first = (int)in_first; p.in_count = (int)in_count;
    p.out_first = (int)out_first; p.nout = (int)nout; p.nch = nch;
    p.max_period = h->max_period; p.span = h->span;
    HIPCHK(h, pv_launch_psola(p, h->stream));
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_psola_last_error(const pv_psola *h) { return last_error(h); }

int64_t pv_psola_window(float *table, int64_t capacity)
{
    if (capacity < 0 || (capacity > 0 && !table)) return -PV_ERR_ARGUMENT;
    if (capacity > 0) window(table, (size_t)(capacity < PV_PSOLA_WINDOW ? capacity : PV_PSOLA_WINDOW));
    return PV_PSOLA_WINDOW;
}

int pv_psola_create(const pv_psola_config *cfg, pv_psola **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_psola_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_psola_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_psola_create: pv_psola_config.struct_size does not match this library (start from PV_PSOLA_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_psola_create: unknown bits in pv_psola_config.flags (must be 0)");
    if (cfg->max_period < 2 || cfg->max_period > PV_PSOLA_MAX_PERIOD)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_psola_create: max_period %d is outside [2, 4096]", (int)cfg->max_period);
    if (cfg->max_channels < 0 || cfg->max_channels > 65535)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_psola_create: max_channels %d is outside [0, 65535]", (int)cfg->max_channels);
    if (cfg->max_outputs < 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_psola_create: negative max_outputs");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_psola *h = (pv_psola *)calloc(1, sizeof(pv_psola));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_psola_create: out of host memory");
    h->magic = HostTraits<pv_psola>::kMagic;
    h->max_period = cfg->max_period;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    int mo = cfg->max_outputs > 0 ? cfg->max_outputs : kDefaultOutputs;
    if (mo > kMaxOutputs) mo = kMaxOutputs;
    h->max_outputs = (mo + PV_PSOLA_TILE - 1) / PV_PSOLA_TILE * PV_PSOLA_TILE;
    h->device = cfg->device_id;
    h->span = pv_psola_span(h->max_period);
    h->stage_in_pitch = (long long)h->max_outputs + 2 * h->max_period + PV_PSOLA_TAPS;

    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    {
        std::vector<float> P(PV_VARI_TABLE_WORDS, 0.0f), H(PV_PSOLA_WINDOW_WORDS, 0.0f);
        if (pv_vari_prototype(P.data(), PV_VARI_TABLE) != PV_VARI_TABLE) { pv_psola_destroy(h); return fail(kNoHandle, PV_ERR_DEVICE, "pv_psola_create: no prototype table"); }
        window(H.data(), PV_PSOLA_WINDOW);
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

int pv_psola_destroy(pv_psola *h)
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
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_psola_set_stream(pv_psola *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // work queued on the old stream is ordered before the new one's
    h->tab_pending = false;
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_psola_synchronize(pv_psola *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int pv_psola_process_device(pv_psola *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *d_out,
                            int64_t out_first, int64_t nout, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check_process(h, "pv_psola_process_device", d_in, nin, in_stride, nch, grains, ngrains, d_out, out_first, nout, out_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nout == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int r = upload_tables(h, grains, ngrains, out_first, nout);
    if (r != PV_OK) return r;
    return launch(h, d_in, 0, nin, (long)in_stride, nch, ngrains, d_out, out_first, nout, (long)out_stride, 0);
}

int pv_psola_process(pv_psola *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *out, int64_t out_first,
                     int64_t nout, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check_process(h, "pv_psola_process", in, nin, in_stride, nch, grains, ngrains, out, out_first, nout, out_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nout == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int r = upload_tables(h, grains, ngrains, out_first, nout);
    if (r != PV_OK) return r;
    // pieces of max_outputs outputs (whole tiles) through the staging buffers: a piece reads the input max_period + 32 samples to either side of it
    const long long reach = h->max_period + PV_PSOLA_TAPS / 2;
    const size_t ipitch = sizeof(float) * (size_t)(nch > 1 ? in_stride : (nin > 0 ? nin : 1)), opitch = sizeof(float) * (size_t)(nch > 1 ? out_stride : nout);
    for (long long at = 0; at < nout; at += h->max_outputs) {
        const long long m = nout - at < h->max_outputs ? nout - at : h->max_outputs, o = out_first + at;
        long long a = o - reach, b = o + m + reach;
        if (a < 0) a = 0;
        if (b > nin) b = nin;
        if (b < a) b = a;
        if (b > a)
            HIPCHK(h, hipMemcpy2DAsync(h->d_stage_in, sizeof(float) * (size_t)h->stage_in_pitch, in + a, ipitch, sizeof(float) * (size_t)(b - a), nch, hipMemcpyHostToDevice,
                                       h->stream));
        const int lr = launch(h, h->d_stage_in, a, b - a, (long)h->stage_in_pitch, nch, ngrains, h->d_stage_out, o, m, (long)h->max_outputs, at / PV_PSOLA_TILE);
        if (lr != PV_OK) return lr;
        HIPCHK(h, hipMemcpy2DAsync(out + at, opitch, h->d_stage_out, sizeof(float) * (size_t)h->max_outputs, sizeof(float) * (size_t)m, nch, hipMemcpyDeviceToHost,
                                   h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PV_OK;
}

}  // extern "C"
