// pv_resample_capi.hip -- host side of the pv_resample_* entry points of include/phaze_amd.h (band-limited rational resampler).
//
// Owns one resampler's device state -- the tap table (transposed, pv_resample.h), per channel slot the newest T - 1 input samples in two buffers
// that swap roles every launch, and the stream counters (I, J) on the host -- and turns calls into launches of pv_resample_kernels.hip.
// pv_resample_design and pv_resample_count are pure host code: the table the kernels use and the closed form of the output count.
// No CPU compute path: without a HIP device pv_resample_create fails with PV_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../host/pv_host_common.h"
#include "pv_resample.h"

namespace {
constexpr int kMaxTerm = 8192;
constexpr double kBeta = 9.0, kCutoff = 0.91;
constexpr int kHalfWidth = 32;
constexpr long long kPiece = 1LL << 27;            // inputs per launch: outputs (<= 8 x) and every relative index stay inside int32
constexpr size_t kLdsBudget = 64 * 1024;

struct Ratio { int L, M, W, T; };

long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }

// nullptr when (up, down) is acceptable, else why not
const char *reduce(int32_t up, int32_t down, Ratio *r)
{
    if (up <= 0 || down <= 0) return "up and down must be positive";
    const long long g = gcd_ll(up, down);
    const long long L = up / g, M = down / g;
    if (L > kMaxTerm || M > kMaxTerm) return "the reduced ratio has a term above 8192";
    if (L > 8 * M || M > 8 * L) return "the ratio up / down must lie within [1/8, 8]";
    r->L = (int)L; r->M = (int)M;
    r->W = (int)((kHalfWidth * (L > M ? L : M) + L - 1) / L);          // ceil(32 max(1, M / L))
    r->T = 2 * r->W;
    return nullptr;
}

// J(I) = max(0, ceil((I - W) L / M))
long long count_of(const Ratio &r, long long I)
{
    if (I <= r.W) return 0;
    const __int128 num = (__int128)(I - r.W) * r.L;
    return (long long)((num + r.M - 1) / r.M);
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

// rows[phase][i], fp64, every row divided by its own sum
void design_rows(const Ratio &r, std::vector<double> &rows)
{
    const int L = r.L, W = r.W, T = r.T;
    const double s = r.M > r.L ? (double)r.M / (double)r.L : 1.0, fc = kCutoff / s, i0b = bessel_i0(kBeta);
    rows.assign((size_t)L * (size_t)T, 0.0);
    for (int ph = 0; ph < L; ph++) {
        double *row = rows.data() + (size_t)ph * T, sum = 0.0;
        for (int i = 0; i < T; i++) {
            const double t = (double)(i - W + 1) - (double)ph / (double)L;
            if (fabs(t) > (double)W) continue;
            const double u = t / (double)W, a = 1.0 - u * u, x = M_PI * fc * t;
            const double sinc = x == 0.0 ? 1.0 : sin(x) / x;
            row[i] = fc * sinc * bessel_i0(kBeta * sqrt(a > 0.0 ? a : 0.0)) / i0b;
            sum += row[i];
        }
        for (int i = 0; i < T; i++) row[i] /= sum;
    }
}
}  // namespace

struct pv_resample {
    uint32_t magic;
    Ratio r;
    int max_channels, device;
    long long max_samples, stage_out_pitch;
    bool shared;                 // the taps-in-LDS instance
    int lane_stride, tile, span;
    hipStream_t own_stream, stream;
    float *d_taps;               // [T][L]
    float *d_hist[2];            // [max_channels][T - 1] each; d_hist[cur] is the state
    int cur;
    long hist_stride;
    long long I, J;              // input samples consumed, output samples produced since the last reset
    float *d_stage_in, *d_stage_out;
    char err[256];
};

namespace {

PV_HOST_HANDLE(pv_resample, 0x50565253u /* 'PVRS' */, pv_resample_destroy);

// One piece of at most kPiece inputs over channel slots [0, nch): device pointers, asynchronous on h->stream.  Advances (I, J) and the history.
int run_piece(pv_resample *h, const float *d_in, float *d_out, int nch, long long nin, long in_stride, long out_stride, long long *produced)
{
    const Ratio &r = h->r;
    const long long J1 = count_of(r, h->I + nin), nout = J1 - h->J;
    PvResampleParams p;
    memset(&p, 0, sizeof p);
    p.in = d_in; p.out = d_out; p.in_stride = in_stride; p.out_stride = out_stride;
    p.hist_in = h->d_hist[h->cur]; p.hist_out = h->d_hist[h->cur ^ 1]; p.hist_stride = h->hist_stride;
    p.taps = h->d_taps;
    const __int128 pos = (__int128)h->J * r.M;                         // output J sits at input position pos / L
    p.phase0 = (int)(pos % r.L);
    p.n0 = (long long)(pos / r.L) - r.W + 1 - h->I;
    p.L = r.L; p.M = r.M; p.T = r.T;
    p.nin = (int)nin; p.nout = (int)nout; p.nch = nch;
    p.tile = h->tile; p.lane_stride = h->lane_stride; p.span = h->span;
    HIPCHK(h, pv_launch_resample(p, h->shared, h->stream));
    HIPCHK(h, pv_launch_resample_history(p, h->stream));
    h->cur ^= 1;
    h->I += nin;
    h->J = J1;
    *produced = nout;
    return PV_OK;
}

int check_process(pv_resample *h, const char *fn, const void *in, const void *out, int32_t nch, int64_t nin, int64_t in_stride, int64_t out_stride,
                  int64_t out_capacity, long long *total)
{
    if (nch < 0 || nin < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel or sample count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    *total = count_of(h->r, h->I + nin) - h->J;
    if ((nin > 0 && !in) || (*total > 0 && !out)) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (out_capacity < *total)
        return failf(h, PV_ERR_ARGUMENT, "%s: out_capacity %lld is below the %lld samples per channel this call produces", fn, (long long)out_capacity, *total);
    if (nch > 1 && (in_stride < nin || out_stride < *total))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than nin (%lld) or the samples produced (%lld)", fn, (long long)nin, *total);
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_resample_last_error(const pv_resample *h) { return last_error(h); }

int64_t pv_resample_count(int32_t up, int32_t down, int64_t total_in)
{
    Ratio r;
    if (reduce(up, down, &r) || total_in < 0) return -PV_ERR_ARGUMENT;
    return count_of(r, total_in);
}

int64_t pv_resample_design(int32_t up, int32_t down, float *taps, int64_t capacity, int32_t *L, int32_t *M, int32_t *W)
{
    Ratio r;
    if (reduce(up, down, &r) || capacity < 0 || (capacity > 0 && !taps)) return -PV_ERR_ARGUMENT;
    if (L) *L = r.L;
    if (M) *M = r.M;
    if (W) *W = r.W;
    const int64_t n = (int64_t)r.L * r.T;
    if (capacity > 0) {
        std::vector<double> rows;
        design_rows(r, rows);
        for (int64_t k = 0; k < n && k < capacity; k++) taps[k] = (float)rows[(size_t)k];
    }
    return n;
}

int pv_resample_create(const pv_resample_config *cfg, pv_resample **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_resample_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_resample_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_resample_create: pv_resample_config.struct_size does not match this library (start from PV_RESAMPLE_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_resample_create: unknown bits in pv_resample_config.flags (must be 0)");
    Ratio r;
    if (const char *why = reduce(cfg->up, cfg->down, &r)) return failf(kNoHandle, PV_ERR_ARGUMENT, "pv_resample_create: %s", why);
    const int maxch = cfg->max_channels > 0 ? cfg->max_channels : 1;
    const long long maxs = cfg->max_samples > 0 ? cfg->max_samples : 4096;
    if (maxch > 65535) return fail(kNoHandle, PV_ERR_UNSUPPORTED, "max_channels above 65535 (grid.y limit)");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_resample *h = (pv_resample *)calloc(1, sizeof(pv_resample));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_resample_create: out of host memory");
    h->magic = HostTraits<pv_resample>::kMagic;
    h->r = r;
    h->max_channels = maxch; h->max_samples = maxs; h->device = cfg->device_id;
    h->hist_stride = r.T - 1;
    // the taps-in-LDS instance: a thread's outputs lie a multiple of L apart and share a tap row; it needs L <= threads and the table beside the span in LDS
    h->shared = false;
    h->lane_stride = PV_RESAMPLE_THREADS;
    if (r.L <= PV_RESAMPLE_THREADS) {
        const int ls = r.L * (PV_RESAMPLE_THREADS / r.L), tile = PV_RESAMPLE_R * ls;
        const int span = (int)(((long long)(tile - 1) * r.M + r.L - 1) / r.L) + r.T;
        if (pv_resample_lds_bytes(span, true, r.L, r.T) <= kLdsBudget) { h->shared = true; h->lane_stride = ls; }
    }
    h->tile = PV_RESAMPLE_R * h->lane_stride;
    h->span = (int)(((long long)(h->tile - 1) * r.M + r.L - 1) / r.L) + r.T;

    CREATE_CHK(h, hipSetDevice(h->device));
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    {
        std::vector<double> rows;
        design_rows(r, rows);
        std::vector<float> tr((size_t)r.L * (size_t)r.T);
        for (int ph = 0; ph < r.L; ph++)
            for (int i = 0; i < r.T; i++) tr[(size_t)i * r.L + ph] = (float)rows[(size_t)ph * r.T + i];
        CREATE_CHK(h, hipMalloc(&h->d_taps, sizeof(float) * tr.size()));
        CREATE_CHK(h, hipMemcpy(h->d_taps, tr.data(), sizeof(float) * tr.size(), hipMemcpyHostToDevice));
    }
    const size_t hist = sizeof(float) * (size_t)maxch * (size_t)h->hist_stride;
    CREATE_CHK(h, hipMalloc(&h->d_hist[0], hist));
    CREATE_CHK(h, hipMalloc(&h->d_hist[1], hist));
    CREATE_CHK(h, hipMemset(h->d_hist[0], 0, hist));
    CREATE_CHK(h, hipMemset(h->d_hist[1], 0, hist));
    h->stage_out_pitch = (maxs * r.L + r.M - 1) / r.M + 1;              // a piece of max_samples inputs never produces more
    CREATE_CHK(h, hipMalloc(&h->d_stage_in, sizeof(float) * (size_t)maxch * (size_t)maxs));
    CREATE_CHK(h, hipMalloc(&h->d_stage_out, sizeof(float) * (size_t)maxch * (size_t)h->stage_out_pitch));
    *out = h;
    return PV_OK;
}

int pv_resample_destroy(pv_resample *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    void *ptrs[] = {h->d_taps, h->d_hist[0], h->d_hist[1], h->d_stage_in, h->d_stage_out};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    (void)hipGetLastError();
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_resample_reset(pv_resample *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->d_hist[h->cur], 0, sizeof(float) * (size_t)h->max_channels * (size_t)h->hist_stride, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->I = h->J = 0;
    return PV_OK;
}

int pv_resample_set_stream(pv_resample *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // work queued on the old stream is ordered before the new one's
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_resample_synchronize(pv_resample *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int pv_resample_out_count(const pv_resample *h, int64_t nin, int64_t *nout)
{
    if (!live(h) || !nout || nin < 0) return PV_ERR_ARGUMENT;
    *nout = count_of(h->r, h->I + nin) - h->J;
    return PV_OK;
}

int pv_resample_process_device(pv_resample *h, const float *d_in, int32_t nch, int64_t nin, int64_t in_stride, float *d_out, int64_t out_stride,
                               int64_t out_capacity, int64_t *nout)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    long long total = 0;
    const int rc = check_process(h, "pv_resample_process_device", d_in, d_out, nch, nin, in_stride, out_stride, out_capacity, &total);
    if (rc != PV_OK) return rc;
    if (nout) *nout = total;
    if (nch == 0 || nin == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    long long done = 0;
    for (long long at = 0; at < nin; at += kPiece) {
        long long got = 0;
        const int r = run_piece(h, d_in + at, d_out + done, nch, nin - at < kPiece ? nin - at : kPiece, (long)in_stride, (long)out_stride, &got);
        if (r != PV_OK) return r;
        done += got;
    }
    return PV_OK;
}

int pv_resample_process(pv_resample *h, const float *in, int32_t nch, int64_t nin, int64_t in_stride, float *out, int64_t out_stride, int64_t out_capacity,
                        int64_t *nout)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    long long total = 0;
    const int rc = check_process(h, "pv_resample_process", in, out, nch, nin, in_stride, out_stride, out_capacity, &total);
    if (rc != PV_OK) return rc;
    if (nout) *nout = total;
    if (nch == 0 || nin == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // pieces of at most max_samples inputs through the staging buffers: the state carries across pieces exactly as across calls
    const size_t ipitch = sizeof(float) * (size_t)(nch > 1 ? in_stride : nin), opitch = sizeof(float) * (size_t)(nch > 1 ? out_stride : (total > 0 ? total : 1));
    long long done = 0;
    for (long long at = 0; at < nin; at += h->max_samples) {
        const long long n = nin - at < h->max_samples ? nin - at : h->max_samples;
        HIPCHK(h, hipMemcpy2DAsync(h->d_stage_in, sizeof(float) * (size_t)h->max_samples, in + at, ipitch, sizeof(float) * (size_t)n, nch, hipMemcpyHostToDevice,
                                   h->stream));
        long long got = 0;
        const int r = run_piece(h, h->d_stage_in, h->d_stage_out, nch, n, (long)h->max_samples, (long)h->stage_out_pitch, &got);
        if (r != PV_OK) return r;
        if (got > 0)
            HIPCHK(h, hipMemcpy2DAsync(out + done, opitch, h->d_stage_out, sizeof(float) * (size_t)h->stage_out_pitch, sizeof(float) * (size_t)got, nch,
                                       hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        done += got;
    }
    return PV_OK;
}

int pv_resample_export_state(pv_resample *h, int32_t ch, float *hist, int64_t *total_in, int64_t *total_out)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (ch < 0 || ch >= h->max_channels) return fail(h, PV_ERR_CAPACITY, "pv_resample_export_state: channel slot out of range");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hist) HIPCHK(h, hipMemcpy(hist, h->d_hist[h->cur] + (size_t)ch * h->hist_stride, sizeof(float) * (size_t)h->hist_stride, hipMemcpyDeviceToHost));
    if (total_in) *total_in = h->I;
    if (total_out) *total_out = h->J;
    return PV_OK;
}

int pv_resample_import_state(pv_resample *h, int32_t ch, const float *hist, int64_t total_in, int64_t total_out)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (ch < 0 || ch >= h->max_channels) return fail(h, PV_ERR_CAPACITY, "pv_resample_import_state: channel slot out of range");
    if (total_in >= 0 && total_out != count_of(h->r, total_in))
        return fail(h, PV_ERR_ARGUMENT, "pv_resample_import_state: total_out is not the output count of total_in (pv_resample_count)");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hist) HIPCHK(h, hipMemcpy(h->d_hist[h->cur] + (size_t)ch * h->hist_stride, hist, sizeof(float) * (size_t)h->hist_stride, hipMemcpyHostToDevice));
    if (total_in >= 0) { h->I = total_in; h->J = total_out; }
    return PV_OK;
}

}  // extern "C"
