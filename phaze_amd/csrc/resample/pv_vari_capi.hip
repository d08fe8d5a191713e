// pv_vari_capi.hip -- host side of the pv_vari_* entry points of include/phaze_amd.h (variable-ratio band-limited resampler).
//
// Owns one resampler's device state -- the prototype table P, per channel slot the newest T - 1 input samples in two buffers that swap roles every
// launch, and the informational counters (blocks, outputs) on the host -- and turns calls into launches of pv_vari_kernels.hip.  Per launch it
// uploads the prefix sums of the counts and, per tile, the blocks of the tile's first and last output, through a page-locked buffer on the
// handle's stream.  pv_vari_prototype and pv_vari_half_width are pure host code.
// No CPU compute path: without a HIP device pv_vari_create fails with PV_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../host/pv_host_common.h"
#include "pv_resample.h"
#include "pv_vari.h"

namespace {
constexpr double kBeta = 9.0, kCutoff = 0.91;
constexpr int kMaxBlock = 4096, kMaxCount = 8192;
constexpr long long kPieceIn = 1LL << 27;          // inputs per launch: outputs (<= 8 x) and every relative index stay inside int32
constexpr long long kPieceBlocks = 1LL << 24;      // blocks per launch: bounds the uploaded tables (64 MiB of prefix sums)
constexpr size_t kLdsBudget = 64 * 1024;

struct Shape { int B, cmin, cmax, W, T; };

// nullptr when (block, min_count, max_count) is acceptable, else why not
const char *check_shape(int32_t block, int32_t cmin, int32_t cmax, Shape *s)
{
    if (block < 1 || block > kMaxBlock) return "block must lie in [1, 4096]";
    if (cmin < 1 || cmin > cmax || cmax > kMaxCount) return "counts need 1 <= min_count <= max_count <= 8192";
    if (block > 8 * cmin) return "block above 8 * min_count: the step block / count must lie within [1/8, 8]";
    if (cmax > 8 * block) return "max_count above 8 * block: the step block / count must lie within [1/8, 8]";
    s->B = block; s->cmin = cmin; s->cmax = cmax;
    s->W = (PV_VARI_HALF * (block > cmin ? block : cmin) + cmin - 1) / cmin;          // ceil(32 max(1, B / min_count)) <= 256
    s->T = 2 * s->W;
    return nullptr;
}

double bessel_i0(double x)
{
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

// P[q] = f32(h0(q / Q)), h0(t) = 0.91 sinc(0.91 t) I0(9 sqrt(1 - (t / 32)^2)) / I0(9), for q < 32 Q; 0 from 32 Q on
void prototype(float *P, size_t n)
{
    const double i0b = bessel_i0(kBeta);
    for (size_t q = 0; q < n; q++) {
        if (q >= (size_t)PV_VARI_HALF * PV_VARI_Q) { P[q] = 0.0f; continue; }
        const double t = (double)q / (double)PV_VARI_Q, u = t / (double)PV_VARI_HALF, a = 1.0 - u * u, x = M_PI * kCutoff * t;
        const double sinc = x == 0.0 ? 1.0 : sin(x) / x;
        P[q] = (float)(kCutoff * sinc * bessel_i0(kBeta * sqrt(a > 0.0 ? a : 0.0)) / i0b);
    }
}
}  // namespace

struct pv_vari {
    uint32_t magic;
    Shape s;
    int max_channels, device;
    long long max_blocks, stage_out_pitch;
    int tile, span;
    hipStream_t own_stream, stream;
    float *d_table;              // P
    float *d_hist[2];            // [max_channels][T - 1] each; d_hist[cur] is the state
    int cur;
    long hist_stride;
    long long blocks, outputs;   // since the last reset (informational: no position depends on them)
    int *h_tab, *d_tab;          // the launch's tables: prefix[nb + 1] (padded to an even count), then (first, last) block per tile
    size_t htab_cap, tab_cap;    // (in ints)
    hipEvent_t tab_done;
    bool tab_pending;
    float *d_stage_in, *d_stage_out;
    char err[256];
};

namespace {

PV_HOST_HANDLE(pv_vari, 0x50565652u /* 'PVVR' */, pv_vari_destroy);

// One launch of nb blocks (nb B <= kPieceIn, nb <= kPieceBlocks) over channel slots [0, nch): device pointers, asynchronous on h->stream.  Advances history and counters.
int run_piece(pv_vari *h, const float *d_in, float *d_out, int nch, const int32_t *counts, int nb, long in_stride, long out_stride, long long *produced)
{
    const Shape &s = h->s;
    long long total = 0;
    for (int b = 0; b < nb; b++) total += counts[b];
    const int ntiles = (int)((total + h->tile - 1) / h->tile);
    const size_t pre = ((size_t)nb + 2) & ~(size_t)1, words = pre + 2 * (size_t)ntiles;
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
    int *prefix = h->h_tab, *tiles = h->h_tab + pre;
    prefix[0] = 0;
    for (int b = 0; b < nb; b++) prefix[b + 1] = prefix[b] + counts[b];
    for (int t = 0, b = 0; t < ntiles; t++) {
        const long long first = (long long)t * h->tile, last = (first + h->tile < total ? first + h->tile : total) - 1;
        while (prefix[b + 1] <= first) b++;
        tiles[2 * t] = b;
        int e = b;
        while (prefix[e + 1] <= last) e++;
        tiles[2 * t + 1] = e;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_tab, h->h_tab, words * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->tab_done, h->stream));
    h->tab_pending = true;

    PvVariParams p;
    memset(&p, 0, sizeof p);
    p.in = d_in; p.out = d_out; p.in_stride = in_stride; p.out_stride = out_stride;
    p.hist_in = h->d_hist[h->cur]; p.hist_stride = h->hist_stride;
    p.table = h->d_table; p.prefix = h->d_tab; p.tile_blocks = (const int2 *)(h->d_tab + pre);
    p.B = s.B; p.W = s.W; p.T = s.T;
    p.nin = nb * s.B; p.nout = (int)total; p.nch = nch;
    p.tile = h->tile; p.span = h->span;
    HIPCHK(h, pv_launch_vari(p, h->stream));
    PvResampleParams r;                                                   // the history roll of the fixed resampler: the newest T - 1 samples
    memset(&r, 0, sizeof r);
    r.in = d_in; r.in_stride = in_stride; r.hist_in = h->d_hist[h->cur]; r.hist_out = h->d_hist[h->cur ^ 1]; r.hist_stride = h->hist_stride;
    r.T = s.T; r.nin = p.nin; r.nch = nch;
    HIPCHK(h, pv_launch_resample_history(r, h->stream));
    h->cur ^= 1;
    h->blocks += nb;
    h->outputs += total;
    *produced = total;
    return PV_OK;
}

int check_process(pv_vari *h, const char *fn, const void *in, const void *out, int32_t nch, int64_t nblocks, const int32_t *counts, int64_t in_stride,
                  int64_t out_stride, int64_t out_capacity, long long *total)
{
    if (nch < 0 || nblocks < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel or block count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (nblocks > 0 && !counts) return failf(h, PV_ERR_ARGUMENT, "%s: null counts", fn);
    if (nblocks > INT64_MAX / kMaxCount) return failf(h, PV_ERR_ARGUMENT, "%s: too many blocks", fn);
    long long sum = 0;
    for (int64_t b = 0; b < nblocks; b++) {
        if (counts[b] < h->s.cmin || counts[b] > h->s.cmax)
            return failf(h, PV_ERR_ARGUMENT, "%s: count %d of block %lld is outside [min_count %d, max_count %d]", fn, (int)counts[b], (long long)b, h->s.cmin,
                         h->s.cmax);
        sum += counts[b];
    }
    *total = sum;
    const long long nin = (long long)nblocks * h->s.B;
    if ((nin > 0 && !in) || (sum > 0 && !out)) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (out_capacity < sum)
        return failf(h, PV_ERR_ARGUMENT, "%s: out_capacity %lld is below the %lld samples per channel this call produces", fn, (long long)out_capacity, sum);
    if (nch > 1 && (in_stride < nin || out_stride < sum))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the input read (%lld) or the samples produced (%lld)", fn, nin, sum);
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_vari_last_error(const pv_vari *h) { return last_error(h); }

int32_t pv_vari_half_width(int32_t block, int32_t min_count, int32_t max_count)
{
    Shape s;
    if (const char *why = check_shape(block, min_count, max_count, &s)) return -failf(kNoHandle, PV_ERR_ARGUMENT, "pv_vari: %s", why);
    return s.W;
}

int64_t pv_vari_prototype(float *table, int64_t capacity)
{
    if (capacity < 0 || (capacity > 0 && !table)) return -PV_ERR_ARGUMENT;
    if (capacity > 0) prototype(table, (size_t)(capacity < PV_VARI_TABLE ? capacity : PV_VARI_TABLE));
    return PV_VARI_TABLE;
}

int pv_vari_create(const pv_vari_config *cfg, pv_vari **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_vari_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_vari_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_vari_create: pv_vari_config.struct_size does not match this library (start from PV_VARI_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_vari_create: unknown bits in pv_vari_config.flags (must be 0)");
    Shape s;
    if (const char *why = check_shape(cfg->block, cfg->min_count, cfg->max_count, &s)) return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_vari_create: %s", why);
    if (cfg->max_channels < 0 || cfg->max_blocks < 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_vari_create: negative max_channels or max_blocks");
    const int maxch = cfg->max_channels > 0 ? cfg->max_channels : 1;
    long long maxb = cfg->max_blocks > 0 ? cfg->max_blocks : (4096 + s.B - 1) / s.B;
    if (maxb * s.B > kPieceIn) maxb = kPieceIn / s.B;
    if (maxb > kPieceBlocks) maxb = kPieceBlocks;
    if (maxch > 65535) return fail(kNoHandle, PV_ERR_UNSUPPORTED, "max_channels above 65535 (grid.y limit)");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_vari *h = (pv_vari *)calloc(1, sizeof(pv_vari));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_vari_create: out of host memory");
    h->magic = HostTraits<pv_vari>::kMagic;
    h->s = s;
    h->max_channels = maxch; h->max_blocks = maxb; h->device = cfg->device_id;
    h->hist_stride = s.T - 1;
    // the larger of the two tiles whose span, prefix slice and table fit the LDS budget (R = PV_VARI_R - 1 fits every shape: at B = 8 min_count its
    // span is 767 * 8 + 1 + 512 samples, 62.9 KB in all)
    for (int R = PV_VARI_R; R >= PV_VARI_R - 1; R--) {
        h->tile = R * PV_VARI_THREADS;
        h->span = (int)(((long long)(h->tile - 1) * s.B) / s.cmin) + 1 + s.T;
        if (pv_vari_lds_bytes(h->span, h->tile) + 16 <= kLdsBudget) break;
    }

    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    {
        std::vector<float> P(PV_VARI_TABLE_WORDS, 0.0f);
        prototype(P.data(), PV_VARI_TABLE);
        CREATE_CHK(h, hipMalloc(&h->d_table, sizeof(float) * P.size()));
        CREATE_CHK(h, hipMemcpy(h->d_table, P.data(), sizeof(float) * P.size(), hipMemcpyHostToDevice));
    }
    const size_t hist = sizeof(float) * (size_t)maxch * (size_t)h->hist_stride;
    CREATE_CHK(h, hipMalloc(&h->d_hist[0], hist));
    CREATE_CHK(h, hipMalloc(&h->d_hist[1], hist));
    CREATE_CHK(h, hipMemset(h->d_hist[0], 0, hist));
    CREATE_CHK(h, hipMemset(h->d_hist[1], 0, hist));
    h->stage_out_pitch = maxb * s.cmax;
    CREATE_CHK(h, hipMalloc(&h->d_stage_in, sizeof(float) * (size_t)maxch * (size_t)(maxb * s.B)));
    CREATE_CHK(h, hipMalloc(&h->d_stage_out, sizeof(float) * (size_t)maxch * (size_t)h->stage_out_pitch));
    *out = h;
    return PV_OK;
}

int pv_vari_destroy(pv_vari *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->tab_done) (void)hipEventDestroy(h->tab_done);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->h_tab) (void)hipHostFree(h->h_tab);
    void *ptrs[] = {h->d_table, h->d_hist[0], h->d_hist[1], h->d_tab, h->d_stage_in, h->d_stage_out};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    (void)hipGetLastError();
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_vari_reset(pv_vari *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->d_hist[h->cur], 0, sizeof(float) * (size_t)h->max_channels * (size_t)h->hist_stride, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->blocks = h->outputs = 0;
    return PV_OK;
}

int pv_vari_set_stream(pv_vari *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // work queued on the old stream is ordered before the new one's
    h->tab_pending = false;
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_vari_synchronize(pv_vari *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int pv_vari_process_device(pv_vari *h, const float *d_in, int32_t nch, int64_t nblocks, const int32_t *counts, int64_t in_stride, float *d_out,
                           int64_t out_stride, int64_t out_capacity, int64_t *nout)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    long long total = 0;
    const int rc = check_process(h, "pv_vari_process_device", d_in, d_out, nch, nblocks, counts, in_stride, out_stride, out_capacity, &total);
    if (rc != PV_OK) return rc;
    if (nout) *nout = total;
    if (nch == 0 || nblocks == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const long long piece = kPieceIn / h->s.B < kPieceBlocks ? kPieceIn / h->s.B : kPieceBlocks;
    long long done = 0;
    for (long long at = 0; at < nblocks; at += piece) {
        long long got = 0;
        const int r = run_piece(h, d_in + at * h->s.B, d_out + done, nch, counts + at, (int)(nblocks - at < piece ? nblocks - at : piece), (long)in_stride,
                                (long)out_stride, &got);
        if (r != PV_OK) return r;
        done += got;
    }
    return PV_OK;
}

int pv_vari_process(pv_vari *h, const float *in, int32_t nch, int64_t nblocks, const int32_t *counts, int64_t in_stride, float *out, int64_t out_stride,
                    int64_t out_capacity, int64_t *nout)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    long long total = 0;
    const int rc = check_process(h, "pv_vari_process", in, out, nch, nblocks, counts, in_stride, out_stride, out_capacity, &total);
    if (rc != PV_OK) return rc;
    if (nout) *nout = total;
    if (nch == 0 || nblocks == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // pieces of at most max_blocks blocks through the staging buffers: the state carries across pieces exactly as across calls
    const long long nin = (long long)nblocks * h->s.B, spitch = h->max_blocks * h->s.B;
    const size_t ipitch = sizeof(float) * (size_t)(nch > 1 ? in_stride : nin), opitch = sizeof(float) * (size_t)(nch > 1 ? out_stride : (total > 0 ? total : 1));
    long long done = 0;
    for (long long at = 0; at < nblocks; at += h->max_blocks) {
        const long long nb = nblocks - at < h->max_blocks ? nblocks - at : h->max_blocks;
        HIPCHK(h, hipMemcpy2DAsync(h->d_stage_in, sizeof(float) * (size_t)spitch, in + at * h->s.B, ipitch, sizeof(float) * (size_t)(nb * h->s.B), nch,
                                   hipMemcpyHostToDevice, h->stream));
        long long got = 0;
        const int r = run_piece(h, h->d_stage_in, h->d_stage_out, nch, counts + at, (int)nb, (long)spitch, (long)h->stage_out_pitch, &got);
        if (r != PV_OK) return r;
        HIPCHK(h, hipMemcpy2DAsync(out + done, opitch, h->d_stage_out, sizeof(float) * (size_t)h->stage_out_pitch, sizeof(float) * (size_t)got, nch,
                                   hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        done += got;
    }
    return PV_OK;
}

int pv_vari_export_state(pv_vari *h, int32_t ch, float *hist, int64_t *total_blocks, int64_t *total_out)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (ch < 0 || ch >= h->max_channels) return fail(h, PV_ERR_CAPACITY, "pv_vari_export_state: channel slot out of range");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hist) HIPCHK(h, hipMemcpy(hist, h->d_hist[h->cur] + (size_t)ch * h->hist_stride, sizeof(float) * (size_t)h->hist_stride, hipMemcpyDeviceToHost));
    if (total_blocks) *total_blocks = h->blocks;
    if (total_out) *total_out = h->outputs;
    return PV_OK;
}

int pv_vari_import_state(pv_vari *h, int32_t ch, const float *hist, int64_t total_blocks, int64_t total_out)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (ch < 0 || ch >= h->max_channels) return fail(h, PV_ERR_CAPACITY, "pv_vari_import_state: channel slot out of range");
    if (total_blocks >= 0 && total_out < 0) return fail(h, PV_ERR_ARGUMENT, "pv_vari_import_state: negative total_out");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hist) HIPCHK(h, hipMemcpy(h->d_hist[h->cur] + (size_t)ch * h->hist_stride, hist, sizeof(float) * (size_t)h->hist_stride, hipMemcpyHostToDevice));
    if (total_blocks >= 0) { h->blocks = total_blocks; h->outputs = total_out; }
    return PV_OK;
}

}  // extern "C"
