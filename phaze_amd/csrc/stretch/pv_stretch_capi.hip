// pv_stretch_capi.hip -- host side of the pv_stretch_* entry points of include/phaze_amd.h (phase-locked time stretch).
//
// Owns one time-stretch handle's device state -- per channel slot hist[N - ha] | acc[N - hs] | phi[H] | psi[H] (pv_stretch.h) -- and turns calls
// into pass A + scan + pass B launches (pv_stretch_kernels.hip).  No CPU compute path: without a HIP device pv_stretch_create fails with PV_ERR_DEVICE.
// pv_tempo_process / pv_tempo_process_device (variable tempo) turn a host schedule of per-frame hops into the kernels' position table.
// pv_link_channels groups consecutive slots: a linked handle runs the LINK instances of the passes (one phase track per group).
// pv_transient_process / pv_transient_process_device add a host row of per-frame reset flags (the RESET instances), uploaded as prefix counts behind
// the position table; pv_onset_strength runs the stateless detection kernel of pv_onset_kernels.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../host/pv_host_common.h"
#include "pv_stretch.h"

struct pv_stretch {
    uint32_t magic;
    int N, log2n, ha, hs, H, halo;
    int max_channels, max_frames, device, cus;
    hipStream_t own_stream, stream;
    double2 *d_tw64;
    float2 *d_tw32;
    float *d_hann;
    long stride;                 // floats per channel slot of the state
    float *d_state, *d_state_out;
    unsigned *d_sums;            // pass A / scan / pass B exchange, grown on demand
    size_t sums_cap;             // (in u32 words)
    float *d_stage_in, *d_stage_out;   // host-pointer calls: max_channels x max_frames frames
    long stage_in_pitch;         // floats per channel of d_stage_in: max_frames * ha, or N once a tempo call needed one frame of hop N to fit
    long long *d_pos, *h_pos;    // variable tempo: the position table on the device, and its page-locked upload buffer (grown on demand)
    size_t pos_cap, hpos_cap;    // (in int64 words)
    hipEvent_t pos_done;         // recorded behind the last upload: h_pos may be rewritten once it has completed
    bool pos_pending;
    int *d_rst;                  // phase resets: the prefix counts of the last upload, inside d_pos behind the position table
    float *d_onset_in;           // pv_onset_strength on host pointers: the whole buffer and its counts, grown on demand
    int *d_onset_counts;
    size_t onset_in_cap, onset_counts_cap;   // (in words)
    int group;                   // channels per linked group (pv_link_channels), 1: unlinked
    char err[256];
};

namespace {

PV_HOST_HANDLE(pv_stretch, 0x50565453u /* 'PVTS' */, pv_stretch_destroy);

// Frames per chain: one round of the workgroups the chip holds at once (each takes `lds` + `pad` bytes of a CU's LDS, at most 8 per CU) over `groups`
// rows of the grid, but never fewer than min_frames.
int chain_frames(const pv_stretch *h, size_t lds, size_t pad, int groups, int nframes, long min_frames)
{
    long per_cu = (long)((160 * 1024) / (lds + pad));
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    long chains = per_cu * h->cus / (groups > 0 ? groups : 1);
    if (chains < 1) chains = 1;
    long F = (nframes + chains - 1) / chains;
    if (F < min_frames) F = min_frames;
    if (F > nframes) F = nframes;
    return (int)F;
}

// the stretch passes: never fewer than four times the (halo + 1) frames a chain recomputes
int pick_chain(const pv_stretch *h, int groups, int nframes)
{
    return chain_frames(h, pv_stretch_lds_bytes(h->log2n, true), 512, groups, nframes, 4L * (h->halo + 1));
}

// the onset kernel: at least 8 frames (each chain transforms one extra frame, m0 - 1)
int onset_chain(const pv_stretch *h, int groups, int nframes)
{
    return chain_frames(h, pv_stretch_lds_bytes(h->log2n, false), 2048, groups, nframes, 8);
}

// One launch over channel slots [0, nch): device pointers, asynchronous on h->stream.  d_pos: the position table of a tempo call (pv_stretch.h), or
// nullptr for the fixed hop.  d_rst: the reset prefix counts of a transient call (needs d_pos), or nullptr.
int run(pv_stretch *h, const float *d_in, float *d_out, int nch, int nframes, long in_stride, long out_stride, const long long *d_pos = nullptr,
        long pos_stride = 0, const int *d_rst = nullptr, long rst_stride = 0)
{
    PvStretchParams p;
    memset(&p, 0, sizeof p);
    p.in = d_in; p.out = d_out; p.in_stride = in_stride; p.out_stride = out_stride;
    p.nframes = nframes; p.nch = nch; p.ha = h->ha; p.hs = h->hs;
    p.F = pick_chain(h, nch / h->group, nframes);                      // linked: chains enough to fill the chip with pass A's nch / G workgroups
    p.nchains = (nframes + p.F - 1) / p.F;
    p.halo = h->halo;
    p.ola_scale = (float)((double)h->hs / (double)h->N);
    p.state_in = h->d_state; p.state_out = h->d_state_out; p.state_stride = h->stride;
    p.tw64 = h->d_tw64; p.tw32 = h->d_tw32; p.hann = h->d_hann;
    p.pos = d_pos; p.pos_stride = pos_stride;
    const int rc = grow(h, &h->d_sums, &h->sums_cap, (size_t)(nch / h->group) * (size_t)p.nchains * 2 * (size_t)h->H);
    if (rc != PV_OK) return rc;
    p.sums = h->d_sums;
    HIPCHK(h, pv_launch_stretch(h->log2n, p, h->group, d_rst, rst_stride, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_state, h->d_state_out, sizeof(float) * (size_t)nch * (size_t)h->stride, hipMemcpyDeviceToDevice, h->stream));
    return PV_OK;
}

// What every call checks first: the two buffers, the counts, the capacity, whole linked groups.  fn: the name the message opens with.
int check_buffers(pv_stretch *h, const char *fn, const void *a, const void *b, int32_t nch, int32_t nframes)
{
    if (!a || !b) return failf(h, PV_ERR_ARGUMENT, "%s: null buffer", fn);
    if (nch < 0 || nframes < 0) return failf(h, PV_ERR_ARGUMENT, "%s: negative channel or frame count", fn);
    if (nch > h->max_channels) return failf(h, PV_ERR_CAPACITY, "%s: more channels than max_channels", fn);
    if (nch % h->group != 0)
        return failf(h, PV_ERR_ARGUMENT, "%s: %d channels are not a whole number of linked groups of %d", fn, nch, h->group);
    return PV_OK;
}

int check_call(pv_stretch *h, const void *in, const void *out, int32_t nch, int32_t nframes, int64_t in_stride, int64_t out_stride)
{
    const int rc = check_buffers(h, "pv_stretch_process", in, out, nch, nframes);
    if (rc != PV_OK) return rc;
    if (nch > 1 && (in_stride < (int64_t)nframes * h->ha || out_stride < (int64_t)nframes * h->hs))
        return fail(h, PV_ERR_ARGUMENT, "pv_stretch_process: channel strides shorter than nframes * hop");
    return PV_OK;
}

// ---- variable tempo ----

// Everything a tempo call may reject, before any device work.  tot[r]: the input total of schedule row r (nrows = 1 for a shared row, else nch).
int check_tempo(pv_stretch *h, const char *fn, const void *in, const void *out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
                int64_t in_stride, int64_t out_stride, std::vector<long long> &tot, const uint8_t *resets = nullptr, int64_t reset_stride = 0)
{
    const int rc = check_buffers(h, fn, in, out, nch, nframes);
    if (rc != PV_OK) return rc;
    if (nframes > 0 && !hops) return failf(h, PV_ERR_ARGUMENT, "%s: null hops", fn);
    if (hop_stride != 0 && hop_stride < nframes)
        return failf(h, PV_ERR_ARGUMENT, "%s: hop_stride %lld is neither 0 (one row for every channel) nor >= nframes %d", fn, (long long)hop_stride, nframes);
    const int nrows = hop_stride == 0 ? 1 : nch;
    tot.assign((size_t)nrows, 0);
    long long most = 0;
    for (int r = 0; r < nrows && nframes > 0; r++) {
        const int32_t *row = hops + (size_t)r * (size_t)hop_stride;
        long long t = 0;
        for (int m = 0; m < nframes; m++) {
            if (row[m] < h->ha || row[m] > h->N)
                return failf(h, PV_ERR_ARGUMENT, "%s: hop %d of channel %d, frame %d is outside [analysis_hop %d, fft_size %d]", fn, (int)row[m], r, m, h->ha, h->N);
            t += row[m];
        }
        tot[(size_t)r] = t;
        if (t > most) most = t;
    }
    // linked channels share their group's phase track and so its schedule: every row of a group must equal the group's first
    for (int r = 0; r < nrows && nrows > 1 && nframes > 0; r++) {
        if (r % h->group == 0) continue;
        const int32_t *row = hops + (size_t)r * (size_t)hop_stride, *first = hops + (size_t)(r - r % h->group) * (size_t)hop_stride;
        for (int m = 0; m < nframes; m++)
            if (row[m] != first[m])
                return failf(h, PV_ERR_ARGUMENT, "%s: schedule rows differ within linked group %d (channels %d .. %d): channel %d, frame %d", fn, r / h->group,
                         r - r % h->group, r - r % h->group + h->group - 1, r, m);
    }
    if (resets) {
        if (reset_stride != 0 && reset_stride < nframes)
            return failf(h, PV_ERR_ARGUMENT, "%s: reset_stride %lld is neither 0 (one row for every channel) nor >= nframes %d", fn, (long long)reset_stride, nframes);
        const int rrows = reset_stride == 0 ? 1 : nch;
        for (int r = 0; r < rrows; r++) {
            const uint8_t *row = resets + (size_t)r * (size_t)reset_stride, *first = resets + (size_t)(r - r % h->group) * (size_t)reset_stride;
            for (int m = 0; m < nframes; m++) {
                if (row[m] > 1)
                    return failf(h, PV_ERR_ARGUMENT, "%s: reset flag %d of channel %d, frame %d is neither 0 nor 1", fn, (int)row[m], r, m);
                if (row[m] != first[m])
                    return failf(h, PV_ERR_ARGUMENT, "%s: reset rows differ within linked group %d (channels %d .. %d): channel %d, frame %d", fn, r / h->group,
                             r - r % h->group, r - r % h->group + h->group - 1, r, m);
            }
        }
    }
    if (nch > 1 && (in_stride < most || out_stride < (int64_t)nframes * h->hs))
        return failf(h, PV_ERR_ARGUMENT, "%s: channel strides shorter than the largest row's input (%lld) or nframes * synthesis_hop (%lld)", fn, most,
                 (long long)nframes * h->hs);
    return PV_OK;
}

// Frames [f0, f0 + nf) of every row as a position table, S[r][i] = sum of hops f0 .. f0 + i - 1 of row r, uploaded on h->stream into h->d_pos.
// The page-locked h_pos is rewritten only once the previous upload has completed, so a device call may follow another before any synchronise.
// With resets: the flags of the same frames as int32 prefix counts, R[r][0] = 0, R[r][i + 1] = R[r][i] + flag, packed behind the table in the same
// upload; h->d_rst then points at them (rrows rows of nf + 1).
int upload_pos(pv_stretch *h, const int32_t *hops, int64_t hop_stride, int nrows, int f0, int nf, const uint8_t *resets = nullptr, int64_t reset_stride = 0,
               int rrows = 0)
{
    const size_t pos_words = (size_t)nrows * (size_t)(nf + 1);
    const size_t words = pos_words + (resets ? ((size_t)rrows * (size_t)(nf + 1) + 1) / 2 : 0);      // two int32 counts per int64 word
    if (h->pos_pending) HIPCHK(h, hipEventSynchronize(h->pos_done));
    h->pos_pending = false;
    if (words > h->hpos_cap) {
        if (h->h_pos) (void)hipHostFree(h->h_pos);
        h->h_pos = nullptr; h->hpos_cap = 0;
        HIPCHK(h, hipHostMalloc((void **)&h->h_pos, words * sizeof(long long), hipHostMallocDefault));
        h->hpos_cap = words;
    }
    const int rc = grow(h, &h->d_pos, &h->pos_cap, words);
    if (rc != PV_OK) return rc;
    if (!h->pos_done) HIPCHK(h, hipEventCreateWithFlags(&h->pos_done, hipEventDisableTiming));
    for (int r = 0; r < nrows; r++) {
        const int32_t *row = hops + (size_t)r * (size_t)hop_stride + f0;
        long long *S = h->h_pos + (size_t)r * (size_t)(nf + 1);
        S[0] = 0;
        for (int i = 0; i < nf; i++) S[i + 1] = S[i] + row[i];
    }
    h->d_rst = nullptr;
    if (resets) {
        int *R0 = (int *)(h->h_pos + pos_words);
        for (int r = 0; r < rrows; r++) {
            const uint8_t *row = resets + (size_t)r * (size_t)reset_stride + f0;
            int *R = R0 + (size_t)r * (size_t)(nf + 1);
            R[0] = 0;
            for (int i = 0; i < nf; i++) R[i + 1] = R[i] + row[i];
        }
        h->d_rst = (int *)(h->d_pos + pos_words);
    }
    HIPCHK(h, hipMemcpyAsync(h->d_pos, h->h_pos, words * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->pos_done, h->stream));
    h->pos_pending = true;
    return PV_OK;
}

}  // namespace

extern "C" {

const char *pv_stretch_last_error(const pv_stretch *h) { return last_error(h); }

int pv_stretch_create(const pv_stretch_config *cfg, pv_stretch **out)
{
    if (!cfg || !out) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_stretch_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(pv_stretch_config))
        return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_stretch_create: pv_stretch_config.struct_size does not match this library (start from PV_STRETCH_CONFIG_INIT)");
    if (cfg->flags != 0) return fail(kNoHandle, PV_ERR_ARGUMENT, "pv_stretch_create: unknown bits in pv_stretch_config.flags (must be 0)");
    const int N = cfg->fft_size, ha = cfg->analysis_hop, hs = cfg->synthesis_hop;
    if (N <= 1 || (N & (N - 1)) != 0) return fail(kNoHandle, PV_ERR_FFT_SIZE, "FFT size must be a power of two and bigger than 1");
    int log2n = 0;
    while ((1 << log2n) < N) log2n++;
    if (!pv_stretch_supported(log2n)) return fail(kNoHandle, PV_ERR_UNSUPPORTED, "fft_size must be within 256..8192 for the time-stretch kernels");
    if (ha < 1 || ha > N) return fail(kNoHandle, PV_ERR_ARGUMENT, "analysis_hop must be within 1..fft_size");
    if (hs < 1 || hs > N / 2) return fail(kNoHandle, PV_ERR_ARGUMENT, "synthesis_hop must be within 1..fft_size/2 (at least two overlapping frames, R_s = N / hs >= 2)");
    const int maxch = cfg->max_channels > 0 ? cfg->max_channels : 1;
    const int maxfr = cfg->max_frames > 0 ? cfg->max_frames : 1;
    if (maxch > 65535) return fail(kNoHandle, PV_ERR_UNSUPPORTED, "max_channels above 65535 (grid.y limit)");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(kNoHandle, PV_ERR_DEVICE, "no HIP device available (this library has no CPU path)"); }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(kNoHandle, PV_ERR_ARGUMENT, "device_id out of range");

    pv_stretch *h = (pv_stretch *)calloc(1, sizeof(pv_stretch));
    if (!h) return fail(kNoHandle, PV_ERR_DEVICE, "pv_stretch_create: out of host memory");
    h->magic = HostTraits<pv_stretch>::kMagic;
    h->N = N; h->log2n = log2n; h->ha = ha; h->hs = hs; h->H = N / 2 + 1; h->halo = (N - 1) / hs;
    h->max_channels = maxch; h->max_frames = maxfr; h->device = cfg->device_id;
    h->group = 1;
    h->stride = pv_stretch_state_stride(N, ha, hs);

    CREATE_CHK(h, hipSetDevice(h->device));
    hipDeviceProp_t prop;
    CREATE_CHK(h, hipGetDeviceProperties(&prop, h->device));
    h->cus = prop.multiProcessorCount;
    CREATE_CHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    CREATE_CHK(h, upload_tables(N, false, &h->d_tw64, &h->d_tw32, &h->d_hann));      // the pitch path's tables (pv_capi.hip), without the half window
    const size_t state = sizeof(float) * (size_t)maxch * (size_t)h->stride;
    CREATE_CHK(h, hipMalloc(&h->d_state, state));
    CREATE_CHK(h, hipMalloc(&h->d_state_out, state));
    CREATE_CHK(h, hipMemset(h->d_state, 0, state));
    CREATE_CHK(h, hipMalloc(&h->d_stage_in, sizeof(float) * (size_t)maxch * (size_t)maxfr * ha));
    h->stage_in_pitch = (long)maxfr * ha;
    CREATE_CHK(h, hipMalloc(&h->d_stage_out, sizeof(float) * (size_t)maxch * (size_t)maxfr * hs));
    *out = h;
    return PV_OK;
}

int pv_stretch_destroy(pv_stretch *h)
{
    if (!h) return PV_ERR_ARGUMENT;
    if (!live(h)) return PV_ERR_DESTROYED;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    if (h->pos_done) (void)hipEventDestroy(h->pos_done);
    void *ptrs[] = {h->d_tw64, h->d_tw32, h->d_hann, h->d_state, h->d_state_out, h->d_sums, h->d_stage_in, h->d_stage_out, h->d_pos, h->d_onset_in,
                    h->d_onset_counts};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_pos) (void)hipHostFree(h->h_pos);
    (void)hipGetLastError();
    h->magic = 0;
    free(h);
    return PV_OK;
}

int pv_stretch_reset(pv_stretch *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(h->d_state, 0, sizeof(float) * (size_t)h->max_channels * (size_t)h->stride, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int pv_link_channels(pv_stretch *h, int32_t channels_per_group)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (channels_per_group < 1 || channels_per_group > h->max_channels)
        return failf(h, PV_ERR_ARGUMENT, "pv_link_channels: channels_per_group %d outside [1, max_channels %d]", (int)channels_per_group, h->max_channels);
    const int rc = pv_stretch_reset(h);                                // per-channel and per-group phases mean different things
    if (rc != PV_OK) return rc;
    h->group = channels_per_group;
    return PV_OK;
}

int pv_stretch_set_stream(pv_stretch *h, void *hip_stream)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));                          // work queued on the old stream is ordered before the new one's
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return PV_OK;
}

int pv_stretch_synchronize(pv_stretch *h)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

int pv_stretch_process_device(pv_stretch *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes, int64_t in_stride, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check_call(h, d_in, d_out, nch, nframes, in_stride, out_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return run(h, d_in, d_out, nch, nframes, (long)in_stride, (long)out_stride);
}

int pv_stretch_process(pv_stretch *h, const float *in, float *out, int32_t nch, int32_t nframes, int64_t in_stride, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check_call(h, in, out, nch, nframes, in_stride, out_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // pieces of at most max_frames frames through the staging buffers: the state carries across pieces exactly as across calls
    const long sin = (long)h->max_frames * h->ha, sout = (long)h->max_frames * h->hs;
    const size_t ipitch = sizeof(float) * (size_t)(nch > 1 ? in_stride : (int64_t)nframes * h->ha);
    const size_t opitch = sizeof(float) * (size_t)(nch > 1 ? out_stride : (int64_t)nframes * h->hs);
    for (int f0 = 0; f0 < nframes; f0 += h->max_frames) {
        const int nf = nframes - f0 < h->max_frames ? nframes - f0 : h->max_frames;
        HIPCHK(h, hipMemcpy2DAsync(h->d_stage_in, sizeof(float) * sin, in + (long)f0 * h->ha, ipitch,
                                   sizeof(float) * (size_t)nf * h->ha, nch, hipMemcpyHostToDevice, h->stream));
        const int r = run(h, h->d_stage_in, h->d_stage_out, nch, nf, sin, sout);
        if (r != PV_OK) return r;
        HIPCHK(h, hipMemcpy2DAsync(out + (long)f0 * h->hs, opitch, h->d_stage_out, sizeof(float) * sout,
                                   sizeof(float) * (size_t)nf * h->hs, nch, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return PV_OK;
}

}  // extern "C"

namespace {

// pv_tempo_process_device, and with `resets` (a host row of 0 / 1 per frame, the row rule of hops) pv_transient_process_device.  transient: the
// entry point takes hops == NULL for "every hop equals the floor, as one shared row"
int tempo_device(pv_stretch *h, const char *fn, bool transient, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops,
                 int64_t hop_stride, const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    std::vector<int32_t> flat;
    if (transient && !hops && nframes > 0) { flat.assign((size_t)nframes, h->ha); hops = flat.data(); hop_stride = 0; }
    std::vector<long long> tot;
    const int rc = check_tempo(h, fn, d_in, d_out, nch, nframes, hops, hop_stride, in_stride, out_stride, tot, resets, reset_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int nrows = hop_stride == 0 ? 1 : nch, rrows = reset_stride == 0 ? 1 : nch;
    const int r = upload_pos(h, hops, hop_stride, nrows, 0, nframes, resets, reset_stride, rrows);
    if (r != PV_OK) return r;
    return run(h, d_in, d_out, nch, nframes, (long)in_stride, (long)out_stride, h->d_pos, hop_stride == 0 ? 0 : (long)nframes + 1, h->d_rst,
               reset_stride == 0 ? 0 : (long)nframes + 1);
}

// pv_tempo_process, and with `resets` pv_transient_process
int tempo_host(pv_stretch *h, const char *fn, bool transient, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops,
               int64_t hop_stride, const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    std::vector<int32_t> flat;
    if (transient && !hops && nframes > 0) { flat.assign((size_t)nframes, h->ha); hops = flat.data(); hop_stride = 0; }
    std::vector<long long> tot;
    const int rc = check_tempo(h, fn, in, out, nch, nframes, hops, hop_stride, in_stride, out_stride, tot, resets, reset_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->stage_in_pitch < h->N) {                                    // max_frames * ha < N: one frame of hop N must fit a piece
        size_t cap = 0;                                                // (regrown whatever it holds)
        const int rg = grow(h, &h->d_stage_in, &cap, (size_t)h->max_channels * (size_t)h->N);
        if (rg != PV_OK) return rg;
        h->stage_in_pitch = h->N;
    }
    // pieces of at most max_frames frames whose every row fits the input staging; each channel row is copied over exactly its own span
    const int nrows = hop_stride == 0 ? 1 : nch, rrows = reset_stride == 0 ? 1 : nch;
    const long sin = h->stage_in_pitch, sout = (long)h->max_frames * h->hs;
    const size_t opitch = sizeof(float) * (size_t)(nch > 1 ? out_stride : (int64_t)nframes * h->hs);
    std::vector<long long> at((size_t)nrows, 0), span((size_t)nrows);    // per row: input consumed before the piece, and the piece's own
    for (int f0 = 0; f0 < nframes;) {
        int nf = 0;
        std::fill(span.begin(), span.end(), 0LL);
        while (nf < h->max_frames && f0 + nf < nframes) {               // the first frame always fits: hop <= N <= sin
            bool fits = true;
            for (int r = 0; r < nrows && fits; r++) fits = span[(size_t)r] + hops[(size_t)r * (size_t)hop_stride + f0 + nf] <= sin;
            if (!fits) break;
            for (int r = 0; r < nrows; r++) span[(size_t)r] += hops[(size_t)r * (size_t)hop_stride + f0 + nf];
            nf++;
        }
        if (nrows == 1) {
            const size_t ipitch = sizeof(float) * (size_t)(nch > 1 ? in_stride : tot[0]);
            HIPCHK(h, hipMemcpy2DAsync(h->d_stage_in, sizeof(float) * sin, in + at[0], ipitch, sizeof(float) * (size_t)span[0], nch,
                                       hipMemcpyHostToDevice, h->stream));
        } else {
            for (int c = 0; c < nch; c++)
                HIPCHK(h, hipMemcpyAsync(h->d_stage_in + (size_t)c * sin, in + (size_t)c * (size_t)in_stride + at[(size_t)c], sizeof(float) * (size_t)span[(size_t)c],
                                         hipMemcpyHostToDevice, h->stream));
        }
        int r = upload_pos(h, hops, hop_stride, nrows, f0, nf, resets, reset_stride, rrows);
        if (r != PV_OK) return r;
        r = run(h, h->d_stage_in, h->d_stage_out, nch, nf, sin, sout, h->d_pos, hop_stride == 0 ? 0 : (long)nf + 1, h->d_rst,
                reset_stride == 0 ? 0 : (long)nf + 1);
        if (r != PV_OK) return r;
        HIPCHK(h, hipMemcpy2DAsync(out + (long)f0 * h->hs, opitch, h->d_stage_out, sizeof(float) * sout,
                                   sizeof(float) * (size_t)nf * h->hs, nch, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int rr = 0; rr < nrows; rr++) at[(size_t)rr] += span[(size_t)rr];
        f0 += nf;
    }
    return PV_OK;
}

int check_onset(pv_stretch *h, const char *fn, const void *in, const void *counts, int32_t nch, int32_t nframes, int64_t in_stride, int64_t count_stride)
{
    const int rc = check_buffers(h, fn, in, counts, nch, nframes);
    if (rc != PV_OK) return rc;
    if ((nch > 1 && in_stride < (int64_t)nframes * h->ha) || (nch > h->group && count_stride < nframes))
        return failf(h, PV_ERR_ARGUMENT, "%s: in_stride below nframes * analysis_hop (%lld) or count_stride below nframes (%d)", fn, (long long)nframes * h->ha, nframes);
    return PV_OK;
}

}  // namespace

extern "C" {

int pv_tempo_process_device(pv_stretch *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
                            int64_t in_stride, int64_t out_stride)
{
    return tempo_device(h, "pv_tempo_process_device", false, d_in, d_out, nch, nframes, hops, hop_stride, nullptr, 0, in_stride, out_stride);
}

int pv_tempo_process(pv_stretch *h, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
                     int64_t in_stride, int64_t out_stride)
{
    return tempo_host(h, "pv_tempo_process", false, in, out, nch, nframes, hops, hop_stride, nullptr, 0, in_stride, out_stride);
}

// hops == NULL: every hop equals the floor, as one shared row
int pv_transient_process_device(pv_stretch *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
                                const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride)
{
    return tempo_device(h, "pv_transient_process_device", true, d_in, d_out, nch, nframes, hops, hop_stride, resets, reset_stride, in_stride, out_stride);
}

int pv_transient_process(pv_stretch *h, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
                         const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride)
{
    return tempo_host(h, "pv_transient_process", true, in, out, nch, nframes, hops, hop_stride, resets, reset_stride, in_stride, out_stride);
}

int pv_onset_strength_device(pv_stretch *h, const float *d_in, int32_t nch, int32_t nframes, int64_t in_stride, int32_t *d_counts, int64_t count_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    const int rc = check_onset(h, "pv_onset_strength_device", d_in, d_counts, nch, nframes, in_stride, count_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, pv_launch_onset_strength(h->log2n, d_in, (long)in_stride, nch, h->group, nframes, h->ha, onset_chain(h, nch / h->group, nframes), h->d_tw64,
                                       h->d_hann, d_counts, (long)count_stride, h->stream));
    return PV_OK;
}

int pv_onset_strength(pv_stretch *h, const float *in, int32_t nch, int32_t nframes, int64_t in_stride, int32_t *counts, int64_t count_stride)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    int rc = check_onset(h, "pv_onset_strength", in, counts, nch, nframes, in_stride, count_stride);
    if (rc != PV_OK) return rc;
    if (nch == 0 || nframes == 0) return PV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int groups = nch / h->group;
    const size_t n = (size_t)nframes * (size_t)h->ha;
    if ((rc = grow(h, &h->d_onset_in, &h->onset_in_cap, (size_t)nch * n)) != PV_OK) return rc;
    if ((rc = grow(h, &h->d_onset_counts, &h->onset_counts_cap, (size_t)groups * (size_t)nframes)) != PV_OK) return rc;
    HIPCHK(h, hipMemcpy2DAsync(h->d_onset_in, sizeof(float) * n, in, sizeof(float) * (size_t)(nch > 1 ? in_stride : (int64_t)n), sizeof(float) * n, nch,
                               hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, pv_launch_onset_strength(h->log2n, h->d_onset_in, (long)n, nch, h->group, nframes, h->ha, onset_chain(h, groups, nframes), h->d_tw64, h->d_hann,
                                       h->d_onset_counts, nframes, h->stream));
    HIPCHK(h, hipMemcpy2DAsync(counts, sizeof(int32_t) * (size_t)(groups > 1 ? count_stride : (int64_t)nframes), h->d_onset_counts, sizeof(int32_t) * (size_t)nframes,
                               sizeof(int32_t) * (size_t)nframes, groups, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PV_OK;
}

// TEST HOOK: how a call of nch channels and nframes frames is cut into chains on this chip
int pv_transient_chain_layout(pv_stretch *h, int32_t nch, int32_t nframes, int32_t *frames_per_chain, int32_t *halo)
{
    if (!live(h) || nch < 1 || nframes < 1 || nch % h->group != 0) return PV_ERR_ARGUMENT;
    if (frames_per_chain) *frames_per_chain = pick_chain(h, nch / h->group, nframes);
    if (halo) *halo = h->halo;
    return PV_OK;
}

// TEST HOOK: the frames per chain of an onset-strength call of nch channels and nframes frames on this chip
int pv_onset_chain_layout(pv_stretch *h, int32_t nch, int32_t nframes, int32_t *frames_per_chain)
{
    if (!live(h) || nch < 1 || nframes < 1 || nch % h->group != 0) return PV_ERR_ARGUMENT;
    if (frames_per_chain) *frames_per_chain = onset_chain(h, nch / h->group, nframes);
    return PV_OK;
}

int pv_stretch_export_state(pv_stretch *h, int32_t ch, float *hist, float *acc, uint32_t *phi, uint32_t *psi)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (ch < 0 || ch >= h->max_channels) return fail(h, PV_ERR_CAPACITY, "pv_stretch_export_state: channel slot out of range");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const float *s = h->d_state + (size_t)ch * h->stride;
    const size_t nh = (size_t)(h->N - h->ha), na = (size_t)(h->N - h->hs), H = (size_t)h->H;
    if (hist && nh) HIPCHK(h, hipMemcpy(hist, s, sizeof(float) * nh, hipMemcpyDeviceToHost));
    if (acc && na) HIPCHK(h, hipMemcpy(acc, s + nh, sizeof(float) * na, hipMemcpyDeviceToHost));
    if (phi) HIPCHK(h, hipMemcpy(phi, s + nh + na, sizeof(uint32_t) * H, hipMemcpyDeviceToHost));
    if (psi) HIPCHK(h, hipMemcpy(psi, s + nh + na + H, sizeof(uint32_t) * H, hipMemcpyDeviceToHost));
    return PV_OK;
}

int pv_stretch_import_state(pv_stretch *h, int32_t ch, const float *hist, const float *acc, const uint32_t *phi, const uint32_t *psi)
{
    if (!live(h)) return PV_ERR_ARGUMENT;
    if (ch < 0 || ch >= h->max_channels) return fail(h, PV_ERR_CAPACITY, "pv_stretch_import_state: channel slot out of range");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float *s = h->d_state + (size_t)ch * h->stride;
    const size_t nh = (size_t)(h->N - h->ha), na = (size_t)(h->N - h->hs), H = (size_t)h->H;
    if (hist && nh) HIPCHK(h, hipMemcpy(s, hist, sizeof(float) * nh, hipMemcpyHostToDevice));
    if (acc && na) HIPCHK(h, hipMemcpy(s + nh, acc, sizeof(float) * na, hipMemcpyHostToDevice));
    if (phi) HIPCHK(h, hipMemcpy(s + nh + na, phi, sizeof(uint32_t) * H, hipMemcpyHostToDevice));
    if (psi) HIPCHK(h, hipMemcpy(s + nh + na + H, psi, sizeof(uint32_t) * H, hipMemcpyHostToDevice));
    return PV_OK;
}

}  // extern "C"
