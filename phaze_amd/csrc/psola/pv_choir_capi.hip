// pv_choir_capi.hip -- host side of the pv_choir_* handle entry points of include/phaze_amd.h (full-grain harmony voices on the overlap-add path:
// several differently planned copies of one input, each overlap-added on its own from grains that may be mirrored, warped or both, summed into one output
// by one kernel).
//
// A pv_choir holds what a pv_tsm holds (pv_tsm_capi.hip, whose shape this file has): the two tables of the kernel, the staging buffers of the
// host-pointer form and the page-locked buffer a call's tables go through; it carries no signal state from call to call.  Per call the host validates
// voice_first, the gains and every grain of every voice (pv_choir_check_grains), then works out per voice and tile of the output range the range of
// grains that can overlap the tile and the source range they read inside it (pv_choir_tiles), takes the hull of those source ranges over the voices,
// refuses the call if a tile's hull exceeds the handle's span, and uploads the concatenated grain table, one int2 per tile, one int2 per (tile, voice)
// and the gains on the handle's stream (layout: pv_choir.h).  pv_choir_plan is in pv_choir_plan.hip.
// No CPU compute path: without a HIP device pv_choir_create fails with PV_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../host/pv_host_common.h"
#include "pv_choir.h"

namespace {
constexpr long long kMaxGrains = 1LL << 27;            // bounds the uploaded table (2 GiB of records)
constexpr int kDefaultOutputs = 1 << 16, kMaxOutputs = 1 << 24;
}  // namespace

struct pv_choir {
    uint32_t magic;
    int max_period, max_rate, max_voices, max_channels, max_outputs, device;       // max_outputs: a multiple of the tile
    int span;                    // the longest hull a tile may have
    hipStream_t own_stream, stream;
    float *d_ptable, *d_htable;
    int *h_tab, *d_tab;          // the call's tables (pv_choir.h): grains, {src0, src_count} per tile, {g_first, g_end} per (tile, voice), gains
    size_t htab_cap, tab_cap;    // (in ints)
    hipEvent_t tab_done;
    bool tab_pending;
    float *d_stage_in, *d_stage_out;
    long long stage_in_pitch;
    char err[256];
};

namespace {

PV_HOST_HANDLE(pv_choir, 0x50564348u /* 'PVCH' */, pv_choir_destroy);

// Where the parts of the call's tables begin, in ints.
struct Layout {
    size_t grains, tiles, ranges, gains, words;
    Layout(long long ngrains, long long ntiles, int nvoices, int nch)
    {
        grains = 0;
        tiles = 4 * (size_t)(ngrains > 0 ? ngrains : 1);
        ranges = tiles + 2 * (size_t)ntiles;
        gains = ranges + 2 * (size_t)ntiles * (size_t)nvoices;
        words = gains + (size_t)nvoices * (size_t)nch;
    }
};

// What both forms check before any device work.
int check_process(pv_choir *h, const char *fn, const void *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, const int64_t *voice_first,
                  int32_t nvoices, const float *gains, const void *out, int64_t out_first, int64_t nout, int64_t out_stride)
{
    if (nch < 0 || nin < 0 || nout < 0 || out_first < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel, sample or output count", fn);
    if (nvoices < 1) return failf(h, PV_ERR_ARGUMENT, "%s: nvoices %d is below 1", fn, (int)nvoices);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (nvoices > h->max_voices) return failf(h, PV_ERR_CAPACITY, "%s: more voices (%d) than max_voices %d", fn, (int)nvoices, h->max_voices);
    if (nin > PV_TSM_MAX_POSITION || out_first > PV_TSM_MAX_POSITION || nout > PV_TSM_MAX_POSITION || out_first + nout > PV_TSM_MAX_POSITION)
        return failf(h, PV_ERR_ARGUMENT, "%s: positions must stay below 2^30", fn);
    if (!voice_first || (nch > 0 && !gains)) return failf(h, PV_ERR_ARGUMENT, "%s: null voice_first or gains", fn);
    if (voice_first[0] != 0) return failf(h, PV_ERR_ARGUMENT, "%s: voice_first[0] is %lld, not 0", fn, (long long)voice_first[0]);
    for (int32_t v = 0; v < nvoices; v++)
        if (voice_first[v + 1] < voice_first[v])
            return failf(h, PV_ERR_ARGUMENT, "%s: voice_first[%d] = %lld lies below voice_first[%d] = %lld (voice %d would have a negative grain count)", fn, (int)v + 1,
                         (long long)voice_first[v + 1], (int)v, (long long)voice_first[v], (int)v);
    const int64_t ngrains = voice_first[nvoices];
    if (ngrains > kMaxGrains) return failf(h, PV_ERR_ARGUMENT, "%s: more than 2^27 grains in one call", fn);
    if ((ngrains > 0 && !grains) || (nch > 0 && nin > 0 && !in) || (nch > 0 && nout > 0 && !out)) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch > 1 && (in_stride < nin || out_stride < nout))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the input (%lld) or the outputs (%lld)", fn, (long long)nin, (long long)nout);
    for (int32_t v = 0; v < nvoices; v++)
        for (int32_t c = 0; c < nch; c++)
            if (!isfinite(gains[(size_t)v * (size_t)nch + (size_t)c]))
                return failf(h, PV_ERR_ARGUMENT, "%s: voice %d: its gain on channel %d is not finite", fn, (int)v, (int)c);
    for (int32_t v = 0; v < nvoices; v++) {
        int why = 0;                                                         // centres may restart at a voice boundary: every voice is checked on its own
        const int32_t *table = voice_first[v + 1] > voice_first[v] ? grains + 4 * voice_first[v] : nullptr;
        const long long k = (long long)pv_choir_check_grains(table, voice_first[v + 1] - voice_first[v], h->max_period, &why);     // counted within its voice
        if (k < 0) continue;
        const int32_t t = table[4 * k], w = table[4 * k + 1], D = table[4 * k + 2], L = table[4 * k + 3];
        switch (why) {
        case PV_CHOIR_BAD_CENTRE:
            return failf(h, PV_ERR_ARGUMENT, "%s: voice %d grain %lld: centre %d is outside [0, 2^30)", fn, (int)v, k, (int)t);
        case PV_CHOIR_BAD_STEP:
            return failf(h, PV_ERR_ARGUMENT, "%s: voice %d grain %lld: its word %d is outside [0, 2^27) or its step %d is neither 0 nor within [128, 512]", fn, (int)v, k,
                         (int)w, (int)((w >> PV_CHOIR_STEP_SHIFT) & 1023));
        case PV_CHOIR_BAD_LENGTH:
            return failf(h, PV_ERR_ARGUMENT, "%s: voice %d grain %lld: half length %d is outside [2, max_period %d]", fn, (int)v, k, (int)L, h->max_period);
        case PV_CHOIR_BAD_SHIFT:
            return failf(h, PV_ERR_ARGUMENT, "%s: voice %d grain %lld: displacement %d is not above -2^30, or not below 2^30 on a forward grain", fn, (int)v, k, (int)D);
        default:
            return failf(h, PV_ERR_ARGUMENT, "%s: voice %d grain %lld: its centre lies before the centre of grain %lld (out of order)", fn, (int)v, k, k - 1);
        }
    }
    return PV_OK;
}

// The call's tables in the page-locked buffer.  Pure host work (the previous upload of the buffer is waited for first); refuses the call when a tile's
// hull exceeds the span.  *longest: the longest hull among the tiles.
int make_tables(pv_choir *h, const char *fn, const int32_t *grains, const int64_t *voice_first, int nvoices, const float *gains, int nch, long long out_first,
                long long nout, int *longest)
{
    const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE, ngrains = voice_first[nvoices];
    const Layout at(ngrains, ntiles, nvoices, nch);
    // the page-locked table is rewritten only once the previous upload has completed, so a device call may follow another before any synchronise
    if (h->tab_pending) HIPCHK(h, hipEventSynchronize(h->tab_done));
    h->tab_pending = false;
    if (at.words > h->htab_cap) {
        if (h->h_tab) (void)hipHostFree(h->h_tab);
        h->h_tab = nullptr; h->htab_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->h_tab, at.words * sizeof(int), hipHostMallocDefault));
        h->htab_cap = at.words;
    }
    int *tiles = h->h_tab + at.tiles, *ranges = h->h_tab + at.ranges;
    // pv_choir_tiles on every voice's own table: {g_first, g_end, src0, src_count} per (voice, tile), the grain indices counted within the voice
    std::vector<int64_t> walk((size_t)nvoices * (size_t)ntiles * 4);
    for (int v = 0; v < nvoices; v++)
        (void)pv_choir_tiles(voice_first[v + 1] > voice_first[v] ? grains + 4 * voice_first[v] : nullptr, voice_first[v + 1] - voice_first[v], h->max_period, out_first,
                             nout, walk.data() + (size_t)v * (size_t)ntiles * 4);
    *longest = 0;
    for (long long t = 0; t < ntiles; t++) {
        const long long j0 = out_first + t * PV_TSM_TILE, j1 = j0 + (nout - t * PV_TSM_TILE < PV_TSM_TILE ? nout - t * PV_TSM_TILE : PV_TSM_TILE);
        long long s0 = 0, s1 = 0, low_grain = 0;
        int low_voice = -1;                                                 // the lowest voice with a grain on the tile
        for (int v = 0; v < nvoices; v++) {
            const int64_t *w = walk.data() + ((size_t)v * (size_t)ntiles + (size_t)t) * 4;
            if (w[3] > 0) {                                                 // a grain of the voice reaches the tile: its range goes into the hull
                if (low_voice < 0 || w[2] < s0) s0 = w[2];
                if (low_voice < 0 || w[2] + w[3] > s1) s1 = w[2] + w[3];
                if (low_voice < 0) { low_voice = v; low_grain = w[0]; }
            }
            ranges[2 * (t * nvoices + v)] = (int)(voice_first[v] + w[0]);
            ranges[2 * (t * nvoices + v) + 1] = (int)(voice_first[v] + w[1]);
        }
        if (s1 - s0 > h->span)
            return failf(h, PV_ERR_ARGUMENT, "%s: tile %lld: voice %d grain %lld: the tile of outputs [%lld, %lld) that begins with it reads %lld input samples over its "
                         "voices, more than the span %d of max_period %d and max_rate %d", fn, t, low_voice, low_grain, j0, j1, s1 - s0, h->span, h->max_period, h->max_rate);
        if (s1 - s0 > *longest) *longest = (int)(s1 - s0);
        tiles[2 * t] = pv_choir_src0(s0);                                   // its low 32 bits: the one corner where it leaves int32 holds zeros (pv_choir.h)
        tiles[2 * t + 1] = (int)(s1 - s0);
    }
    memset(h->h_tab, 0, 4 * sizeof(int));
    if (ngrains > 0) memcpy(h->h_tab, grains, 4 * sizeof(int) * (size_t)ngrains);
    if (nch > 0) memcpy(h->h_tab + at.gains, gains, sizeof(float) * (size_t)nvoices * (size_t)nch);
    return PV_OK;
}

// Uploads what make_tables made.  Asynchronous on h->stream.
int upload_tables(pv_choir *h, long long ngrains, long long nout, int nvoices, int nch)
{
    const Layout at(ngrains, (nout + PV_TSM_TILE - 1) / PV_TSM_TILE, nvoices, nch);
    const int rc = grow(h, &h->d_tab, &h->tab_cap, at.words);
    if (rc != PV_OK) return rc;
    if (!h->tab_done) HIPCHK(h, hipEventCreateWithFlags(&h->tab_done, hipEventDisableTiming));
    HIPCHK(h, hipMemcpyAsync(h->d_tab, h->h_tab, at.words * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->tab_done, h->stream));
    h->tab_pending = true;
    return PV_OK;
}

// One launch: outputs [out_first, out_first + nout) of the call whose tables are uploaded for `call_nout` outputs; tile0 is the index of the launch's
// first tile in them, `longest` the longest hull of the call's tiles (the launch's LDS is sized by it: a multiple of 64 samples, at least two rows of warped taps).
int launch(pv_choir *h, const float *d_in, long long in_first, long long in_count, long in_stride, int nch, long long ngrains, int nvoices, long long call_nout,
           float *d_out, long long out_first, long long nout, long out_stride, long long tile0, int longest)
{
    const Layout at(ngrains, (call_nout + PV_TSM_TILE - 1) / PV_TSM_TILE, nvoices, nch);
    PvChoirParams p;
    memset(&p, 0, sizeof p);
    p.in = d_in; p.out = d_out; p.in_stride = in_stride; p.out_stride = out_stride;
    p.ptable = h->d_ptable; p.htable = h->d_htable;
    p.grains = (const int4 *)(h->d_tab + at.grains);
    p.tiles = (const int2 *)(h->d_tab + at.tiles) + tile0;
    p.ranges = (const int2 *)(h->d_tab + at.ranges) + tile0 * nvoices;
    p.gains = (const float *)(h->d_tab + at.gains);
    p.in_first = in_first; p.in_count = in_count;
    p.out_first = (int)out_first; p.nout = (int)nout; p.nch = nch; p.nvoices = nvoices;
    int span = (longest + 63) & ~63;
    if (span > h->span) span = h->span;                                  // the largest pair of a rate fills the LDS to within 64 samples: no rounding past it
    if (span < 2 * PV_CHOIR_TAPS) span = 2 * PV_CHOIR_TAPS;
    p.span = span;
    HIPCHK(h, pv_launch_choir(p, h->stream));
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_choir_last_error(const pv_choir *h) { return last_error(h); }

int pv_choir_create(const pv_choir_config *cfg, pv_choir **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_choir_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_choir_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_choir_create: pv_choir_config.struct_size does not match this library (start from PV_CHOIR_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_choir_create: unknown bits in pv_choir_config.flags (must be 0)");
    if (cfg->max_period < 2 || cfg->max_period > PV_TSM_MAX_PERIOD)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_choir_create: max_period %d is outside [2, 4096]", (int)cfg->max_period);
    if (cfg->max_rate < 1 || cfg->max_rate > PV_TSM_MAX_RATE)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_choir_create: max_rate %d is outside [1, 4]", (int)cfg->max_rate);
    if (cfg->max_voices < 0 || cfg->max_voices > PV_CHOIR_MAX_VOICES)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_choir_create: max_voices %d is outside [0, %d]", (int)cfg->max_voices, PV_CHOIR_MAX_VOICES);
    if (cfg->max_channels < 0 || cfg->max_channels > 65535)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_choir_create: max_channels %d is outside [0, 65535]", (int)cfg->max_channels);
    if (cfg->max_outputs < 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_choir_create: negative max_outputs");
    const int span = pv_choir_span(cfg->max_period, cfg->max_rate);
    if (pv_tsm_lds_bytes(span) > PV_TSM_LDS_BYTES)
        return failf(kNoHandle, PV_ERR_UNSUPPORTED, "pv_choir_create: max_period %d at max_rate %d stages %d samples per tile: %lld bytes of LDS with the tables, more "
                     "than the %d of a compute unit", (int)cfg->max_period, (int)cfg->max_rate, span, (long long)pv_tsm_lds_bytes(span), PV_TSM_LDS_BYTES);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_choir *h = (pv_choir *)calloc(1, sizeof(pv_choir));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_choir_create: out of host memory");
    h->magic = HostTraits<pv_choir>::kMagic;
    h->max_period = cfg->max_period;
    h->max_rate = cfg->max_rate;
    h->max_voices = cfg->max_voices > 0 ? cfg->max_voices : PV_CHOIR_MAX_VOICES;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    int mo = cfg->max_outputs > 0 ? cfg->max_outputs : kDefaultOutputs;
    if (mo > kMaxOutputs) mo = kMaxOutputs;
    h->max_outputs = (mo + PV_TSM_TILE - 1) / PV_TSM_TILE * PV_TSM_TILE;
    h->device = cfg->device_id;
    h->span = span;
    // what a piece of max_outputs outputs reads when it runs at max_rate, and never less than one tile's span
    h->stage_in_pitch = (long long)h->max_rate * ((long long)h->max_outputs + 2 * h->max_period) + 6 * h->max_period + 192;

    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    {
        std::vector<float> P(PV_VARI_TABLE_WORDS, 0.0f), H(PV_TSM_WINDOW_WORDS, 0.0f);
        if (pv_vari_prototype(P.data(), PV_VARI_TABLE) != PV_VARI_TABLE || pv_psola_window(H.data(), PV_TSM_WINDOW) != PV_TSM_WINDOW) {
            pv_choir_destroy(h);
            return fail(kNoHandle, PV_ERR_DEVICE, "pv_choir_create: no prototype or window table");
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

int pv_choir_destroy(pv_choir *h)
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

int pv_choir_set_stream(pv_choir *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // work queued on the old stream is ordered before the new one's
    h->tab_pending = false;
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_choir_synchronize(pv_choir *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int pv_choir_process_device(pv_choir *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, const int64_t *voice_first,
                              int32_t nvoices, const float *gains, float *d_out, int64_t out_first, int64_t nout, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const char *fn = "pv_choir_process_device";
    const int rc = check_process(h, fn, d_in, nin, in_stride, nch, grains, voice_first, nvoices, gains, d_out, out_first, nout, out_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nout == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int longest = 0;
    int r = make_tables(h, fn, grains, voice_first, nvoices, gains, nch, out_first, nout, &longest);
    if (r != PV_OK) return r;
    const long long ngrains = voice_first[nvoices];
    r = upload_tables(h, ngrains, nout, nvoices, nch);
    if (r != PV_OK) return r;
    return launch(h, d_in, 0, nin, (long)in_stride, nch, ngrains, nvoices, nout, d_out, out_first, nout, (long)out_stride, 0, longest);
}

int pv_choir_process(pv_choir *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, const int64_t *voice_first,
                       int32_t nvoices, const float *gains, float *out, int64_t out_first, int64_t nout, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const char *fn = "pv_choir_process";
    const int rc = check_process(h, fn, in, nin, in_stride, nch, grains, voice_first, nvoices, gains, out, out_first, nout, out_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nout == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    int longest = 0;
    int r = make_tables(h, fn, grains, voice_first, nvoices, gains, nch, out_first, nout, &longest);
    if (r != PV_OK) return r;
    const long long ngrains = voice_first[nvoices];
    r = upload_tables(h, ngrains, nout, nvoices, nch);
    if (r != PV_OK) return r;
    // Pieces of whole tiles through the staging buffers, as pv_tsm_process: a piece stages the hull of its tiles cut to the input.  It takes as many
    // tiles as fit max_outputs and whose hull fits the staging buffer, and always at least one: one tile's hull is at most the span, which the buffer
    // holds.
    const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE, most = h->max_outputs / PV_TSM_TILE;
    const int *tiles = h->h_tab + Layout(ngrains, ntiles, nvoices, nch).tiles;
    const size_t ipitch = sizeof(float) * (size_t)(nch > 1 ? in_stride : (nin > 0 ? nin : 1)), opitch = sizeof(float) * (size_t)(nch > 1 ? out_stride : nout);
    for (long long t0 = 0; t0 < ntiles;) {
        long long a = 0, b = 0, t1 = t0;
        bool any = false;
        while (t1 < ntiles && t1 - t0 < most) {
            long long na = a, nb = b;
            bool nany = any;
            if (tiles[2 * t1 + 1] > 0) {
                long long s0 = tiles[2 * t1], s1 = s0 + tiles[2 * t1 + 1];
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
        const int lr = launch(h, h->d_stage_in, a, b - a, (long)h->stage_in_pitch, nch, ngrains, nvoices, nout, h->d_stage_out, o, m, (long)h->max_outputs, t0, longest);
        if (lr != PV_OK) return lr;
        HIPCHK(h, hipMemcpy2DAsync(out + at, opitch, h->d_stage_out, sizeof(float) * (size_t)h->max_outputs, sizeof(float) * (size_t)m, nch, hipMemcpyDeviceToHost,
                                   h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        t0 = t1;
    }
    return PV_OK;
}

}  // extern "C"
