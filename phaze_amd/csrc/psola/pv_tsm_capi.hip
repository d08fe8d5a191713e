// pv_tsm_capi.hip -- host side of the pv_tsm_* handle entry points of include/phaze_amd.h (time-scale modification by pitch-synchronous overlap-add).
//
// A pv_tsm holds the two tables of the kernel (the prototype P of the variable-ratio resampler and the window table Hn), the staging buffers of the
// host-pointer form and the page-locked buffer a call's tables go through; it carries no signal state from call to call.  Per call the host validates
// every grain, then works out per tile of the output range the contiguous range of grains that can overlap the tile (pv_psola_capi.hip's walk) and the
// source range those grains read inside the tile (pv_tsm.h), refuses the call if a tile's range exceeds the handle's span, and uploads the grain table
// and one int4 per tile on the handle's stream.  pv_tsm_plan is in pv_tsm_plan.hip.
// No CPU compute path: without a HIP device pv_tsm_create fails with PV_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../host/pv_host_common.h"
#include "pv_tsm.h"

namespace {
constexpr long long kMaxGrains = 1LL << 27;            // bounds the uploaded table (2 GiB of records)
constexpr int kDefaultOutputs = 1 << 16, kMaxOutputs = 1 << 24;
}  // namespace

struct pv_tsm {
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
    char err[256];
};

namespace {

PV_HOST_HANDLE(pv_tsm, 0x50565453u /* 'PVTS' */, pv_tsm_destroy);

// What both forms check before any device work.
int check_process(pv_tsm *h, const char *fn, const void *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, const void *out,
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
    long long prev = 0;
    for (int64_t g = 0; g < ngrains; g++) {
        const int32_t t = grains[4 * g], w = grains[4 * g + 1], D = grains[4 * g + 2], L = grains[4 * g + 3];
        if (t < 0 || t >= PV_TSM_MAX_POSITION || w < 0 || w >= PV_TSM_Q * PV_TSM_Q)
            return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: centre %d is outside [0, 2^30) or its fractions %d outside [0, 65535]", fn, (long long)g, (int)t, (int)w);
        if (L < 2 || L > h->max_period) return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: half length %d is outside [2, max_period %d]", fn, (long long)g, (int)L, h->max_period);
        if (D <= -PV_TSM_MAX_POSITION || D >= PV_TSM_MAX_POSITION)
            return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: displacement %d is not inside +-2^30", fn, (long long)g, (int)D);
        const long long c = (long long)t * PV_TSM_Q + (w & (PV_TSM_Q - 1));
        if (c < prev) return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: its centre lies before the centre of grain %lld (out of order)", fn, (long long)g, (long long)g - 1);
        prev = c;
    }
    return PV_OK;
}

// The call's tables in the page-locked buffer: the grains, then per tile of [out_first, out_first + nout) the grain range and the source range.  Pure host
// work (the previous upload of the buffer is waited for first); refuses the call when a tile's source range exceeds the span.  *longest: the longest
// source range among the tiles.
int make_tables(pv_tsm *h, const char *fn, const int32_t *grains, long long ngrains, long long out_first, long long nout, int *longest)
{
    const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE;
    const size_t gw = 4 * (size_t)(ngrains > 0 ? ngrains : 1), words = gw + 4 * (size_t)ntiles;
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
    const long long mp = h->max_period;
    long long lo = 0, hi = 0;
    *longest = 0;
    for (long long t = 0; t < ntiles; t++) {
        const long long j0 = out_first + t * PV_TSM_TILE, j1 = j0 + (nout - t * PV_TSM_TILE < PV_TSM_TILE ? nout - t * PV_TSM_TILE : PV_TSM_TILE);
        // centres are in order and no half length is above max_period: a grain that reaches [j0, j1) has its centre t within [j0 - mp - 1, j1 + mp)
        while (lo < ngrains && grains[4 * lo] < j0 - mp - 1) lo++;
        if (hi < lo) hi = lo;
        while (hi < ngrains && grains[4 * hi] < j1 + mp) hi++;
        long long a = lo, b = hi;                                       // trimmed to the first and the last grain that reach the tile
        while (a < b && (long long)grains[4 * a] + 1 + grains[4 * a + 3] <= j0) a++;
        while (b > a && (long long)grains[4 * (b - 1)] - grains[4 * (b - 1) + 3] >= j1) b--;
        long long s0 = 0, s1 = 0;
        bool any = false;
        for (long long g = a; g < b; g++) {
            const long long c = grains[4 * g], D = grains[4 * g + 2], L = grains[4 * g + 3];
            if (c + L < j0 || c - L >= j1) continue;                    // cannot cover an output of the tile
            const long long from = (j0 > c - L ? j0 : c - L) - D - PV_TSM_TAPS / 2 - 1, to = (j1 < c + L ? j1 : c + L) - D + PV_TSM_TAPS / 2;
            if (!any || from < s0) s0 = from;
            if (!any || to > s1) s1 = to;
            any = true;
        }
        if (s1 - s0 > h->span)
            return failf(h, PV_ERR_ARGUMENT, "%s: grain %lld: the tile of outputs [%lld, %lld) that begins with it reads %lld input samples, more than the span %d of "
                         "max_period %d and max_rate %d", fn, a, j0, j1, s1 - s0, h->span, h->max_period, h->max_rate);
        if (s1 - s0 > *longest) *longest = (int)(s1 - s0);
        tiles[4 * t] = (int)a;
        tiles[4 * t + 1] = (int)b;
        tiles[4 * t + 2] = (int)s0;                                     // within +-(2^31 - 2^20): |D| < 2^30 and positions below 2^30
        tiles[4 * t + 3] = (int)(s1 - s0);
    }
    memset(h->h_tab, 0, 4 * sizeof(int));
    if (ngrains > 0) memcpy(h->h_tab, grains, 4 * sizeof(int) * (size_t)ngrains);
    return PV_OK;
}

// Uploads what make_tables made.  Asynchronous on h->stream.
int upload_tables(pv_tsm *h, long long ngrains, long long nout)
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
int launch(pv_tsm *h, const float *d_in, long long in_first, long long in_count, long in_stride, int nch, long long ngrains, float *d_out, long long out_first,
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
    if (span < 2 * PV_TSM_TAPS) span = 2 * PV_TSM_TAPS;
    p.span = span;
    HIPCHK(h, pv_launch_tsm(p, h->stream));
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_tsm_last_error(const pv_tsm *h) { return last_error(h); }

int pv_tsm_create(const pv_tsm_config *cfg, pv_tsm **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_tsm_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_tsm_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_tsm_create: pv_tsm_config.struct_size does not match this library (start from PV_TSM_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_tsm_create: unknown bits in pv_tsm_config.flags (must be 0)");
    if (cfg->max_period < 2 || cfg->max_period > PV_TSM_MAX_PERIOD)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_tsm_create: max_period %d is outside [2, 4096]", (int)cfg->max_period);
    if (cfg->max_rate < 1 || cfg->max_rate > PV_TSM_MAX_RATE) return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_tsm_create: max_rate %d is outside [1, 4]", (int)cfg->max_rate);
    if (cfg->max_channels < 0 || cfg->max_channels > 65535)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_tsm_create: max_channels %d is outside [0, 65535]", (int)cfg->max_channels);
    if (cfg->max_outputs < 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_tsm_create: negative max_outputs");
    const int span = pv_tsm_span(cfg->max_period, cfg->max_rate);
    if (pv_tsm_lds_bytes(span) > PV_TSM_LDS_BYTES)
        return failf(kNoHandle, PV_ERR_UNSUPPORTED, "pv_tsm_create: max_period %d at max_rate %d stages %d samples per tile: %lld bytes of LDS with the tables, more than the "
                     "%d of a compute unit", (int)cfg->max_period, (int)cfg->max_rate, span, (long long)pv_tsm_lds_bytes(span), PV_TSM_LDS_BYTES);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_tsm *h = (pv_tsm *)calloc(1, sizeof(pv_tsm));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_tsm_create: out of host memory");
    h->magic = HostTraits<pv_tsm>::kMagic;
    h->max_period = cfg->max_period;
    h->max_rate = cfg->max_rate;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    int mo = cfg->max_outputs > 0 ? cfg->max_outputs : kDefaultOutputs;
    if (mo > kMaxOutputs) mo = kMaxOutputs;
    h->max_outputs = (mo + PV_TSM_TILE - 1) / PV_TSM_TILE * PV_TSM_TILE;
    h->device = cfg->device_id;
    h->span = span;
    // what a piece of max_outputs outputs reads when it runs at max_rate, and never less than one tile's span
    h->stage_in_pitch = (long long)h->max_rate * ((long long)h->max_outputs + 2 * h->max_period) + 4 * h->max_period + PV_TSM_TAPS;

    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    {
        std::vector<float> P(PV_VARI_TABLE_WORDS, 0.0f), H(PV_TSM_WINDOW_WORDS, 0.0f);
        if (pv_vari_prototype(P.data(), PV_VARI_TABLE) != PV_VARI_TABLE || pv_psola_window(H.data(), PV_TSM_WINDOW) != PV_TSM_WINDOW) {
            pv_tsm_destroy(h);
            return fail(kNoHandle, PV_ERR_DEVICE, "pv_tsm_create: no prototype or window table");
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

int pv_tsm_destroy(pv_tsm *h)
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

int pv_tsm_set_stream(pv_tsm *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // work queued on the old stream is ordered before the new one's
    h->tab_pending = false;
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_tsm_synchronize(pv_tsm *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int pv_tsm_process_device(pv_tsm *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *d_out,
                          int64_t out_first, int64_t nout, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check_process(h, "pv_tsm_process_device", d_in, nin, in_stride, nch, grains, ngrains, d_out, out_first, nout, out_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nout == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int longest = 0;
    int r = make_tables(h, "pv_tsm_process_device", grains, ngrains, out_first, nout, &longest);
    if (r != PV_OK) return r;
    r = upload_tables(h, ngrains, nout);
    if (r != PV_OK) return r;
    return launch(h, d_in, 0, nin, (long)in_stride, nch, ngrains, d_out, out_first, nout, (long)out_stride, 0, longest);
}

int pv_tsm_process(pv_tsm *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *out, int64_t out_first,
                   int64_t nout, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check_process(h, "pv_tsm_process", in, nin, in_stride, nch, grains, ngrains, out, out_first, nout, out_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nout == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int longest = 0;
    int r = make_tables(h, "pv_tsm_process", grains, ngrains, out_first, nout, &longest);
    if (r != PV_OK) return r;
    r = upload_tables(h, ngrains, nout);
    if (r != PV_OK) return r;
    // Pieces of whole tiles through the staging buffers: a piece stages the input range its tiles read, the union of their source ranges cut to the
    // input.  It takes as many tiles as fit max_outputs and whose union fits the staging buffer, and always at least one: one tile's range is at most
    // the span, which the buffer holds.
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
}

}  // extern "C"
