// pv_takes_capi.hip -- host side of the pv_takes_* entry points of include/phaze_amd.h (per-take plans on the overlap-add path: one call plays K
// independently planned takes of different lengths).
//
// A pv_takes holds what a pv_tsm holds: the two tables of the kernel, the staging buffers of the host-pointer form and the page-locked buffer a call's
// tables go through; it carries no signal state from call to call.  Per call the host validates every take and every grain, walks the tiles of every
// take (pv_tsm_capi.hip's walk, per take: tiles count from the take's own out_first), gives every tile its occupancy class (pv_takes.h), and uploads in
// ONE copy the concatenated grains, the tile records, the tile ids ordered by class and the take records; then one launch per non-empty class.
// pv_takes_tiles is that walk alone, and both process calls run on its records.
// No CPU compute path: without a HIP device pv_takes_create fails with PV_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <new>
#include <vector>

#include "../host/pv_host_common.h"
#include "pv_takes.h"

namespace {
constexpr long long kMaxGrains = 1LL << 27;            // bounds the uploaded table (2 GiB of records)
constexpr int kDefaultOutputs = 1 << 16, kMaxOutputs = 1 << 24;
}  // namespace

struct pv_takes {
    uint32_t magic;
    int max_period, max_rate, max_channels, max_outputs, device;       // max_outputs: a multiple of the tile
    int span;                    // the longest source range a tile may have
    hipStream_t own_stream, stream;
    float *d_ptable, *d_htable;
    int *h_tab, *d_tab;          // the call's tables: grains, tile records, order, take records
    size_t htab_cap, tab_cap;    // (in ints)
    hipEvent_t tab_done;
    bool tab_pending;
    float *d_stage_in, *d_stage_out;
    long long stage_in_pitch;
    std::vector<int32_t> *walked;                                        // pv_takes_tiles's records of the call
    char err[256];
};

namespace {

PV_HOST_HANDLE(pv_takes, 0x5056544Bu /* 'PVTK' */, pv_takes_destroy);

// What create and pv_takes_tiles check of a config before any device is touched.  *span: pv_tsm_span of the pair.
int check_config(const char *fn, const pv_takes_config *cfg, int *span)
{
    if (cfg->struct_size != (int32_t)sizeof(pv_takes_config))
        return failf(kNoHandle, PV_ERR_ARGUMENT, "%s: pv_takes_config.struct_size does not match this library (start from PV_TAKES_CONFIG_INIT)", fn);
    if (cfg->flags != 0) return failf(kNoHandle, PV_ERR_ARGUMENT, "%s: unknown bits in pv_takes_config.flags (must be 0)", fn);
    if (cfg->max_period < 2 || cfg->max_period > PV_TSM_MAX_PERIOD)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "%s: max_period %d is outside [2, 4096]", fn, (int)cfg->max_period);
    if (cfg->max_rate < 1 || cfg->max_rate > PV_TSM_MAX_RATE) return failf(kNoHandle, PV_ERR_ARGUMENT, "%s: max_rate %d is outside [1, 4]", fn, (int)cfg->max_rate);
    if (cfg->max_channels < 0 || cfg->max_channels > 65535)
        return failf(kNoHandle, PV_ERR_ARGUMENT, "%s: max_channels %d is outside [0, 65535]", fn, (int)cfg->max_channels);
    if (cfg->max_outputs < 0) return failf(kNoHandle, PV_ERR_ARGUMENT, "%s: negative max_outputs", fn);
    *span = pv_tsm_span(cfg->max_period, cfg->max_rate);
    if (pv_tsm_lds_bytes(*span) > PV_TSM_LDS_BYTES)
        return failf(kNoHandle, PV_ERR_UNSUPPORTED, "%s: max_period %d at max_rate %d stages %d samples per tile: %lld bytes of LDS with the tables, more than the "
                     "%d of a compute unit", fn, (int)cfg->max_period, (int)cfg->max_rate, *span, (long long)pv_tsm_lds_bytes(*span), PV_TSM_LDS_BYTES);
    return PV_OK;
}

// What every entry point checks of the takes (h == nullptr: pv_takes_tiles, which reports through the create buffer): pv_tsm_process's rules per take,
// and the sums.  in and out are not looked at.
int check_takes(pv_takes *h, const char *fn, int max_period, const pv_take *takes, int32_t ntakes, long long *total_out, long long *total_grains)
{
    if (ntakes < 0 || ntakes > PV_TAKES_MAX_TAKES) return failf(h, PV_ERR_ARGUMENT, "%s: %d takes: outside [0, 65536]", fn, (int)ntakes);
    if (ntakes > 0 && !takes) return failf(h, PV_ERR_ARGUMENT, "%s: null takes", fn);
    long long so = 0, sg = 0;
    for (int k = 0; k < ntakes; k++) {
        const pv_take &t = takes[k];
        if (t.nin < 0 || t.ngrains < 0 || t.nout < 0 || t.out_first < 0) return failf(h, PV_ERR_ARGUMENT, "%s: take %d: negative sample, grain or output count", fn, k);
        if (t.nin > PV_TSM_MAX_POSITION || t.out_first > PV_TSM_MAX_POSITION || t.nout > PV_TSM_MAX_POSITION || t.out_first + t.nout > PV_TSM_MAX_POSITION)
            return failf(h, PV_ERR_ARGUMENT, "%s: take %d: positions must stay below 2^30", fn, k);
        if (t.ngrains > kMaxGrains) return failf(h, PV_ERR_ARGUMENT, "%s: take %d: more than 2^27 grains", fn, k);
        if (t.ngrains > 0 && !t.grains) return failf(h, PV_ERR_ARGUMENT, "%s: take %d: null grains", fn, k);
        so += t.nout; sg += t.ngrains;
        if (so >= PV_TSM_MAX_POSITION) return failf(h, PV_ERR_ARGUMENT, "%s: take %d: the takes' outputs together reach 2^30", fn, k);
        if (sg > kMaxGrains) return failf(h, PV_ERR_ARGUMENT, "%s: take %d: more than 2^27 grains in one call", fn, k);
    }
    for (int k = 0; k < ntakes; k++) {                                  // the tables, once the counts are known to be sane
        const pv_take &t = takes[k];
        const int32_t *grains = t.grains;
        long long prev = 0;
        for (int64_t g = 0; g < t.ngrains; g++) {
            const int32_t c = grains[4 * g], w = grains[4 * g + 1], D = grains[4 * g + 2], L = grains[4 * g + 3];
            if (c < 0 || c >= PV_TSM_MAX_POSITION || w < 0 || w >= PV_TSM_Q * PV_TSM_Q)
                return failf(h, PV_ERR_ARGUMENT, "%s: take %d: grain %lld: centre %d is outside [0, 2^30) or its fractions %d outside [0, 65535]", fn, k, (long long)g, (int)c,
                             (int)w);
            if (L < 2 || L > max_period)
                return failf(h, PV_ERR_ARGUMENT, "%s: take %d: grain %lld: half length %d is outside [2, max_period %d]", fn, k, (long long)g, (int)L, max_period);
            if (D <= -PV_TSM_MAX_POSITION || D >= PV_TSM_MAX_POSITION)
                return failf(h, PV_ERR_ARGUMENT, "%s: take %d: grain %lld: displacement %d is not inside +-2^30", fn, k, (long long)g, (int)D);
            const long long pos = (long long)c * PV_TSM_Q + (w & (PV_TSM_Q - 1));
            if (pos < prev)
                return failf(h, PV_ERR_ARGUMENT, "%s: take %d: grain %lld: its centre lies before the centre of grain %lld (out of order)", fn, k, (long long)g,
                             (long long)g - 1);
            prev = pos;
        }
    }
    *total_out = so; *total_grains = sg;
    return PV_OK;
}

// The tile walk of validated takes: per tile, in (take, tile) order, {take, first, g_first, g_end, src0, src_count, cls, 0} (pv_takes_tiles's record; the
// grain range counts within the take), at most `capacity` of them written.  pv_tsm_capi.hip's walk per take.  Refuses the call when a tile's source range
// exceeds the span.  Returns the number of tiles, or -PV_ERR_*.
long long walk(pv_takes *h, const char *fn, int max_period, int max_rate, int span, const pv_take *takes, int32_t ntakes, int32_t *out, long long capacity)
{
    const long long mp = max_period;
    long long n = 0;
    for (int k = 0; k < ntakes; k++) {
        const int32_t *grains = takes[k].grains;
        const long long ngrains = takes[k].ngrains, out_first = takes[k].out_first, nout = takes[k].nout;
        const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE;
        long long lo = 0, hi = 0;
        for (long long t = 0; t < ntiles; t++, n++) {
            const long long j0 = out_first + t * PV_TSM_TILE, j1 = j0 + (nout - t * PV_TSM_TILE < PV_TSM_TILE ? nout - t * PV_TSM_TILE : PV_TSM_TILE);
            // centres are in order and no half length is above max_period: a grain that reaches [j0, j1) has its centre within [j0 - mp - 1, j1 + mp)
            while (lo < ngrains && grains[4 * lo] < j0 - mp - 1) lo++;
            if (hi < lo) hi = lo;
            while (hi < ngrains && grains[4 * hi] < j1 + mp) hi++;
            long long a = lo, b = hi;                                   // trimmed to the first and the last grain that reach the tile
            while (a < b && (long long)grains[4 * a] + 1 + grains[4 * a + 3] <= j0) a++;
            while (b > a && (long long)grains[4 * (b - 1)] - grains[4 * (b - 1) + 3] >= j1) b--;
            long long s0 = 0, s1 = 0;
            bool any = false;
            for (long long g = a; g < b; g++) {
                const long long c = grains[4 * g], D = grains[4 * g + 2], L = grains[4 * g + 3];
                if (c + L < j0 || c - L >= j1) continue;                // cannot cover an output of the tile
                const long long from = (j0 > c - L ? j0 : c - L) - D - PV_TSM_TAPS / 2 - 1, to = (j1 < c + L ? j1 : c + L) - D + PV_TSM_TAPS / 2;
                if (!any || from < s0) s0 = from;
                if (!any || to > s1) s1 = to;
                any = true;
            }
            if (s1 - s0 > span) {
                failf(h, PV_ERR_ARGUMENT, "%s: take %d: grain %lld: the tile of outputs [%lld, %lld) that begins with it reads %lld input samples, more than the span %d "
                      "of max_period %d and max_rate %d", fn, k, a, j0, j1, s1 - s0, span, max_period, max_rate);
                return -PV_ERR_ARGUMENT;
            }
            if (n < capacity) {
                int32_t *r = out + PV_TAKES_TILE_WORDS * n;
                r[0] = k;
                r[1] = (int32_t)(t * PV_TSM_TILE);
                r[2] = (int32_t)a;
                r[3] = (int32_t)b;
                r[4] = (int32_t)s0;                                     // within +-(2^31 - 2^20): |D| < 2^30 and positions below 2^30
                r[5] = (int32_t)(s1 - s0);
                r[6] = pv_takes_class((int)(s1 - s0));
                r[7] = 0;
            }
        }
    }
    return n;
}

// What the process calls check beyond check_takes: the channels, the buffers, the strides, and that no two output rows overlap.
int check_buffers(pv_takes *h, const char *fn, const pv_take *takes, int32_t ntakes, int32_t nch)
{
    if (nch > 0)
        for (int k = 0; k < ntakes; k++) {
            const pv_take &t = takes[k];
            if ((t.nin > 0 && !t.in) || (t.nout > 0 && !t.out)) return failf(h, PV_ERR_ARGUMENT, "%s: take %d: null buffer", fn, k);
            if (nch > 1 && (t.in_stride < t.nin || t.out_stride < t.nout))
                return failf(h, PV_ERR_ARGUMENT, "%s: take %d: channel strides shorter than the input (%lld) or the outputs (%lld)", fn, k, (long long)t.nin,
                             (long long)t.nout);
        }
    struct Row { uintptr_t a, b; int take; };
    std::vector<Row> rows;
    for (int k = 0; k < ntakes; k++)
        for (int c = 0; c < nch && takes[k].nout > 0; c++) {
            const uintptr_t a = (uintptr_t)(takes[k].out + (long long)c * (nch > 1 ? takes[k].out_stride : 0));
            rows.push_back(Row{a, a + sizeof(float) * (uintptr_t)takes[k].nout, k});
        }
    std::sort(rows.begin(), rows.end(), [](const Row &x, const Row &y) { return x.a < y.a || (x.a == y.a && x.take < y.take); });
    for (size_t i = 1; i < rows.size(); i++)                            // sorted by their first byte: rows overlap if and only if two neighbours do
        if (rows[i].a < rows[i - 1].b)
            return failf(h, PV_ERR_ARGUMENT, "%s: take %d and take %d: their output rows overlap (two workgroups would write the same samples)", fn,
                         std::min(rows[i - 1].take, rows[i].take), std::max(rows[i - 1].take, rows[i].take));
    return PV_OK;
}

// Where the parts of a call's table lie (in ints): grains, then two int4 per tile, then the tile ids, then the take records.
struct Layout {
    size_t grains, tiles, order, recs, words;
    Layout(long long ngrains, long long ntiles, long long nrecs)
    {
        grains = 0;
        tiles = 4 * (size_t)(ngrains > 0 ? ngrains : 1);
        order = tiles + PV_TAKES_TILE_WORDS * (size_t)ntiles;
        recs = (order + (size_t)ntiles + 3) & ~(size_t)3;
        words = recs + PV_TAKES_REC_WORDS * (size_t)nrecs;
    }
};

// The page-locked table, `words` ints, once the previous upload has completed.
int host_table(pv_takes *h, size_t words)
{
    if (h->tab_pending) HIPCHK(h, hipEventSynchronize(h->tab_done));
    h->tab_pending = false;
    if (words > h->htab_cap) {
        if (h->h_tab) (void)hipHostFree(h->h_tab);
        h->h_tab = nullptr; h->htab_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->h_tab, words * sizeof(int), hipHostMallocDefault));
        h->htab_cap = words;
    }
    return PV_OK;
}

int upload_table(pv_takes *h, size_t words)
{
    const int rc = grow(h, &h->d_tab, &h->tab_cap, words);
    if (rc != PV_OK) return rc;
    if (!h->tab_done) HIPCHK(h, hipEventCreateWithFlags(&h->tab_done, hipEventDisableTiming));
    HIPCHK(h, hipMemcpyAsync(h->d_tab, h->h_tab, words * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->tab_done, h->stream));
    h->tab_pending = true;
    return PV_OK;
}

// The concatenated grains into the table; first[k]: where take k's grains begin.
void put_grains(pv_takes *h, const pv_take *takes, int32_t ntakes, std::vector<long long> &first)
{
    memset(h->h_tab, 0, 4 * sizeof(int));
    first.assign((size_t)ntakes + 1, 0);
    for (int k = 0; k < ntakes; k++) {
        if (takes[k].ngrains > 0) memcpy(h->h_tab + 4 * (size_t)first[k], takes[k].grains, 4 * sizeof(int) * (size_t)takes[k].ngrains);
        first[k + 1] = first[k] + takes[k].ngrains;
    }
}

// The device record of the walked tile w: its take record `rec`, whose out_first lies `base` outputs after the take's, and the take's grains from `g0` on.
void put_tile(int *dst, const int32_t *w, int rec, long long base, long long g0, long long nout)
{
    const long long left = nout - w[1];
    dst[0] = rec;
    dst[1] = (int)(w[1] - base);
    dst[2] = (int)(g0 + w[2]);
    dst[3] = (int)(g0 + w[3]);
    dst[4] = w[4];
    dst[5] = w[5];
    dst[6] = (int)(left < PV_TSM_TILE ? left : PV_TSM_TILE);
    dst[7] = 0;
}

void put_rec(int *dst, const float *in, float *out, long long in_stride, long long out_stride, long long in_first, long long in_count, long long out_first)
{
    PvTakeRec r;
    memset(&r, 0, sizeof r);
    r.in = in; r.out = out; r.in_stride = in_stride; r.out_stride = out_stride; r.in_first = in_first; r.in_count = in_count; r.out_first = (int)out_first;
    memcpy(dst, &r, sizeof r);
}

// The tile ids [t0, t1) into order[t0 .. t1), by class, (take, tile) order kept within a class.  count[c - 1], longest[c - 1]: the tiles of class c and the
// longest source range among them.
void put_order(int *order, const int32_t *walked, long long t0, long long t1, long long count[PV_TAKES_CLASSES], int longest[PV_TAKES_CLASSES])
{
    long long at[PV_TAKES_CLASSES];
    for (int c = 0; c < PV_TAKES_CLASSES; c++) { count[c] = 0; longest[c] = 0; }
    for (long long t = t0; t < t1; t++) {
        const int c = walked[PV_TAKES_TILE_WORDS * t + 6] - 1;
        count[c]++;
        if (walked[PV_TAKES_TILE_WORDS * t + 5] > longest[c]) longest[c] = walked[PV_TAKES_TILE_WORDS * t + 5];
    }
    at[0] = t0;
    for (int c = 1; c < PV_TAKES_CLASSES; c++) at[c] = at[c - 1] + count[c - 1];
    for (long long t = t0; t < t1; t++) order[at[walked[PV_TAKES_TILE_WORDS * t + 6] - 1]++] = (int)t;
}

// One launch per non-empty class of the tiles whose ids lie in order[t0 .. t1).
int launch_classes(pv_takes *h, const Layout &lay, long long ngrains, long long ntiles, long long nrecs, int nch, long long t0, const long long count[PV_TAKES_CLASSES],
                   const int longest[PV_TAKES_CLASSES])
{
    long long at = t0;
    for (int c = 0; c < PV_TAKES_CLASSES; c++) {
        if (count[c] > 0) {
            PvTakesParams p;
            memset(&p, 0, sizeof p);
            p.ptable = h->d_ptable; p.htable = h->d_htable;
            p.grains = (const int4 *)(h->d_tab + lay.grains);
            p.tiles = (const int4 *)(h->d_tab + lay.tiles);
            p.order = h->d_tab + lay.order + at;
            p.takes = (const PvTakeRec *)(h->d_tab + lay.recs);
            p.ngrains = (int)ngrains; p.ntiles = (int)ntiles; p.ntakes = (int)nrecs;
            p.count = (int)count[c]; p.nch = nch;
            p.span = pv_takes_launch_span(longest[c]);
            HIPCHK(h, pv_launch_takes(p, h->stream));
        }
        at += count[c];
    }
    return PV_OK;
}

// Validation and walk of a process call.  *ntiles < 0: nothing to do.
int prepare(pv_takes *h, const char *fn, const pv_take *takes, int32_t ntakes, int32_t nch, long long *ntiles, long long *ngrains)
{
    *ntiles = -1;
    if (nch < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    long long total_out = 0;
    int rc = check_takes(h, fn, h->max_period, takes, ntakes, &total_out, ngrains);
    if (rc != PV_OK) return rc;
    rc = check_buffers(h, fn, takes, ntakes, nch);
    if (rc != PV_OK) return rc;
    long long n = 0;
    for (int k = 0; k < ntakes; k++) n += (takes[k].nout + PV_TSM_TILE - 1) / PV_TSM_TILE;
    h->walked->resize(PV_TAKES_TILE_WORDS * (size_t)n);
    const long long got = walk(h, fn, h->max_period, h->max_rate, h->span, takes, ntakes, h->walked->data(), n);
    if (got < 0) return (int)-got;
    if (nch == 0 || total_out == 0) return PV_OK;
    *ntiles = n;
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_takes_last_error(const pv_takes *h) { return last_error(h); }

int pv_takes_create(const pv_takes_config *cfg, pv_takes **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_takes_create: null argument");
    *out = nullptr;
    int span = 0;
    const int rc = check_config("pv_takes_create", cfg, &span);
    if (rc != PV_OK) return rc;

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_takes *h = (pv_takes *)calloc(1, sizeof(pv_takes));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_takes_create: out of host memory");
    h->magic = HostTraits<pv_takes>::kMagic;
    h->walked = new (std::nothrow) std::vector<int32_t>();
    if (!h->walked) { free(h); return fail(kNoHandle, PV_ERR_DEVICE, "pv_takes_create: out of host memory"); }
    h->max_period = cfg->max_period;
    h->max_rate = cfg->max_rate;
    h->max_channels = cfg->max_channels > 0 ? cfg->max_channels : 1;
    int mo = cfg->max_outputs > 0 ? cfg->max_outputs : kDefaultOutputs;
    if (mo > kMaxOutputs) mo = kMaxOutputs;
    h->max_outputs = (mo + PV_TSM_TILE - 1) / PV_TSM_TILE * PV_TSM_TILE;
    h->device = cfg->device_id;
    h->span = span;
    // what a piece of max_outputs outputs reads when it runs at max_rate, and never less than one tile's span (pv_tsm_create's size)
    h->stage_in_pitch = (long long)h->max_rate * ((long long)h->max_outputs + 2 * h->max_period) + 4 * h->max_period + PV_TSM_TAPS;

    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    {
        std::vector<float> P(PV_VARI_TABLE_WORDS, 0.0f), H(PV_TSM_WINDOW_WORDS, 0.0f);
        if (pv_vari_prototype(P.data(), PV_VARI_TABLE) != PV_VARI_TABLE || pv_psola_window(H.data(), PV_TSM_WINDOW) != PV_TSM_WINDOW) {
            pv_takes_destroy(h);
            return fail(kNoHandle, PV_ERR_DEVICE, "pv_takes_create: no prototype or window table");
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

int pv_takes_destroy(pv_takes *h)
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
    delete h->walked;
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_takes_set_stream(pv_takes *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // work queued on the old stream is ordered before the new one's
    h->tab_pending = false;
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_takes_synchronize(pv_takes *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int64_t pv_takes_tiles(const pv_takes_config *cfg, const pv_take *takes, int32_t ntakes, int32_t *tiles, int64_t capacity)
{
    const char *fn = "pv_takes_tiles";
    if (!cfg) return -fail(kNoHandle, PV_ERR_ARGUMENT, "pv_takes_tiles: null config");
    int span = 0;
    int rc = check_config(fn, cfg, &span);
    if (rc != PV_OK) return -rc;
    if (capacity < 0 || (capacity > 0 && !tiles)) return -fail(kNoHandle, PV_ERR_ARGUMENT, "pv_takes_tiles: negative capacity or null tiles");
    long long total_out = 0, total_grains = 0;
    rc = check_takes(kNoHandle, fn, cfg->max_period, takes, ntakes, &total_out, &total_grains);
    if (rc != PV_OK) return -rc;
    return walk(kNoHandle, fn, cfg->max_period, cfg->max_rate, span, takes, ntakes, tiles, capacity);
}

static int process_device_impl(pv_takes *h, const pv_take *takes, int32_t ntakes, int32_t nch)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    long long ntiles = 0, ngrains = 0;
    int rc = prepare(h, "pv_takes_process_device", takes, ntakes, nch, &ntiles, &ngrains);
    if (rc != PV_OK || ntiles < 0) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const Layout lay(ngrains, ntiles, ntakes);
    rc = host_table(h, lay.words);
    if (rc != PV_OK) return rc;
    std::vector<long long> first;
    put_grains(h, takes, ntakes, first);
    const int32_t *walked = h->walked->data();
    for (long long t = 0; t < ntiles; t++) {
        const int k = walked[PV_TAKES_TILE_WORDS * t];
        put_tile(h->h_tab + lay.tiles + PV_TAKES_TILE_WORDS * t, walked + PV_TAKES_TILE_WORDS * t, k, 0, first[k], takes[k].nout);
    }
    long long count[PV_TAKES_CLASSES];
    int longest[PV_TAKES_CLASSES];
    put_order(h->h_tab + lay.order, walked, 0, ntiles, count, longest);
    for (int k = 0; k < ntakes; k++)
        put_rec(h->h_tab + lay.recs + PV_TAKES_REC_WORDS * (size_t)k, takes[k].in, takes[k].out, takes[k].in_stride, takes[k].out_stride, 0, takes[k].nin, takes[k].out_first);
    rc = upload_table(h, lay.words);
    if (rc != PV_OK) return rc;
    return launch_classes(h, lay, ngrains, ntiles, ntakes, nch, 0, count, longest);
}

static int process_impl(pv_takes *h, const pv_take *takes, int32_t ntakes, int32_t nch)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    long long ntiles = 0, ngrains = 0;
    int rc = prepare(h, "pv_takes_process", takes, ntakes, nch, &ntiles, &ngrains);
    if (rc != PV_OK || ntiles < 0) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t *walked = h->walked->data();
    // Pieces: runs of consecutive tiles in (take, tile) order with at most max_outputs outputs, whose takes' hulls (the union of the source ranges of a
    // take's tiles in the piece, cut to the input), laid one after the other, fit the staging buffer.  A piece always holds at least one tile: one
    // tile's range is at most the span, which the buffer holds.  A segment is one take's share of a piece, and has the take record the kernel reads.
    struct Segment { int take; long long t0, t1, a, b, in_at, out_at, nout; };
    struct Piece { long long t0, t1; size_t s0, s1; };
    std::vector<Segment> segs;
    std::vector<Piece> pieces;
    for (long long t0 = 0; t0 < ntiles;) {
        const size_t s_first = segs.size();
        long long t1 = t0, outs = 0, ins = 0;
        while (t1 < ntiles) {
            const int32_t *w = walked + PV_TAKES_TILE_WORDS * t1;
            const int k = w[0];
            const long long left = takes[k].nout - w[1], cnt = left < PV_TSM_TILE ? left : PV_TSM_TILE;
            const bool open = segs.size() > s_first && segs.back().take == k;
            long long a = open ? segs.back().a : 0, b = open ? segs.back().b : 0;
            if (w[5] > 0) {
                long long s0 = w[4], s1 = s0 + w[5];
                if (s0 < 0) s0 = 0;
                if (s1 > takes[k].nin) s1 = takes[k].nin;
                if (s1 > s0) {
                    if (b > a) { a = s0 < a ? s0 : a; b = s1 > b ? s1 : b; }
                    else { a = s0; b = s1; }
                }
            }
            const long long grown = ins - (open ? segs.back().b - segs.back().a : 0) + (b - a);
            if (t1 > t0 && (outs + cnt > h->max_outputs || grown > h->stage_in_pitch)) break;
            if (!open) segs.push_back(Segment{k, t1, t1, 0, 0, 0, outs, 0});
            Segment &s = segs.back();
            s.a = a; s.b = b; s.t1 = t1 + 1; s.nout += cnt;
            ins = grown; outs += cnt;
            t1++;
        }
        long long at = 0;
        for (size_t s = s_first; s < segs.size(); s++) { segs[s].in_at = at; at += segs[s].b - segs[s].a; }
        pieces.push_back(Piece{t0, t1, s_first, segs.size()});
        t0 = t1;
    }
    const Layout lay(ngrains, ntiles, (long long)segs.size());
    rc = host_table(h, lay.words);
    if (rc != PV_OK) return rc;
    std::vector<long long> first;
    put_grains(h, takes, ntakes, first);
    std::vector<long long> count(PV_TAKES_CLASSES * pieces.size());
    std::vector<int> longest(PV_TAKES_CLASSES * pieces.size());
    for (size_t q = 0; q < pieces.size(); q++) {
        for (size_t s = pieces[q].s0; s < pieces[q].s1; s++) {
            const Segment &sg = segs[s];
            const long long base = walked[PV_TAKES_TILE_WORDS * sg.t0 + 1];                 // the segment's first output, relative to the take's
            for (long long t = sg.t0; t < sg.t1; t++)
                put_tile(h->h_tab + lay.tiles + PV_TAKES_TILE_WORDS * t, walked + PV_TAKES_TILE_WORDS * t, (int)s, base, first[sg.take], takes[sg.take].nout);
            put_rec(h->h_tab + lay.recs + PV_TAKES_REC_WORDS * s, h->d_stage_in + sg.in_at, h->d_stage_out + sg.out_at, h->stage_in_pitch, h->max_outputs, sg.a, sg.b - sg.a,
                    takes[sg.take].out_first + base);
        }
        put_order(h->h_tab + lay.order, walked, pieces[q].t0, pieces[q].t1, &count[PV_TAKES_CLASSES * q], &longest[PV_TAKES_CLASSES * q]);
    }
    rc = upload_table(h, lay.words);
    if (rc != PV_OK) return rc;
    for (size_t q = 0; q < pieces.size(); q++) {
        for (size_t s = pieces[q].s0; s < pieces[q].s1; s++) {
            const Segment &sg = segs[s];
            const pv_take &t = takes[sg.take];
            if (sg.b > sg.a)
                HIPCHK(h, hipMemcpy2DAsync(h->d_stage_in + sg.in_at, sizeof(float) * (size_t)h->stage_in_pitch, t.in + sg.a,
                                           sizeof(float) * (size_t)(nch > 1 ? t.in_stride : t.nin), sizeof(float) * (size_t)(sg.b - sg.a), nch, hipMemcpyHostToDevice,
                                           h->stream));
        }
        rc = launch_classes(h, lay, ngrains, ntiles, (long long)segs.size(), nch, pieces[q].t0, &count[PV_TAKES_CLASSES * q], &longest[PV_TAKES_CLASSES * q]);
        if (rc != PV_OK) return rc;
        for (size_t s = pieces[q].s0; s < pieces[q].s1; s++) {
            const Segment &sg = segs[s];
            const pv_take &t = takes[sg.take];
            const long long base = walked[PV_TAKES_TILE_WORDS * sg.t0 + 1];
            HIPCHK(h, hipMemcpy2DAsync(t.out + base, sizeof(float) * (size_t)(nch > 1 ? t.out_stride : t.nout), h->d_stage_out + sg.out_at,
                                       sizeof(float) * (size_t)h->max_outputs, sizeof(float) * (size_t)sg.nout, nch, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PV_OK;
}

// The vectors of a call (the walked tiles, the rows of the overlap check, the pieces) can run out of host memory: no exception leaves the C boundary.
int pv_takes_process_device(pv_takes *h, const pv_take *takes, int32_t ntakes, int32_t nch)
{
    try {
        return process_device_impl(h, takes, ntakes, nch);
    } catch (const std::exception &) {
        return fail(h, PV_ERR_DEVICE, "pv_takes_process_device: out of host memory");
    }
}

int pv_takes_process(pv_takes *h, const pv_take *takes, int32_t ntakes, int32_t nch)
{
    try {
        return process_impl(h, takes, ntakes, nch);
    } catch (const std::exception &) {
        return fail(h, PV_ERR_DEVICE, "pv_takes_process: out of host memory");
    }
}

}  // extern "C"
