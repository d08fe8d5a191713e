/* pv_glide.c -- a pitch curve at constant duration through the C ABI from plain C99: a generated tone through a pv_glide handle (time stretch on a hop
 * row, then the variable-ratio resampler on the same row) along a linear hop ramp, once as one call and once in calls of a few frames on a second
 * handle, and a JSON line with the lengths, the tone's measured frequency ratio over the first and the last quarter next to hs / hop there, and
 * whether the two outputs are the same bits.
 *
 *   cc -std=c99 -I include examples/pv_glide.c -L phaze_amd/lib -lphaze_amd -lm -o pv_glide
 *   ./pv_glide [fft_size synthesis_hop first_hop last_hop nframes]      (default 1024 320 200 400 400: pitch glides from x 1.6 down to x 0.8)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "phaze_amd.h"

static int fail(const char *what, int rc, const pv_glide *h)
{
    fprintf(stderr, "%s: %s (%s)\n", what, pv_status_string(rc), pv_glide_last_error(h));
    return 1;
}

/* positive-going zero crossings per sample over [lo, hi) */
static double crossing_rate(const float *y, long lo, long hi)
{
    long i, first = -1, last = -1, n = 0;
    for (i = lo + 1; i < hi; i++)
        if (y[i - 1] < 0.0f && y[i] >= 0.0f) {
            if (first < 0) first = i;
            last = i;
            n++;
        }
    return n > 1 ? (double)(n - 1) / (double)(last - first) : 0.0;
}

int main(int argc, char **argv)
{
    pv_glide_config cfg = PV_GLIDE_CONFIG_INIT;
    const int N = argc > 1 ? atoi(argv[1]) : 1024;
    const int hs = argc > 2 ? atoi(argv[2]) : 320;
    const int h0 = argc > 3 ? atoi(argv[3]) : 200;
    const int h1 = argc > 4 ? atoi(argv[4]) : 400;
    const int nframes = argc > 5 ? atoi(argv[5]) : 400;
    const double f0 = 441.0 / 48000.0;                     /* cycles per sample */
    pv_glide *a = NULL, *b = NULL;
    float *in, *out, *ref;
    int32_t *hops, W;
    long i, total = 0, done = 0, lag, sum[2] = {0, 0}, lo[2], hi[2];
    double want[2], got[2];
    int m, q, rc, same;
    if (nframes < 8 || h0 < 1 || h1 < 1 || hs < 1 || N < 2) {
        fprintf(stderr, "need nframes >= 8 and positive sizes\n");
        return 2;
    }
    cfg.fft_size = N;
    cfg.synthesis_hop = hs;
    cfg.min_hop = h0 < h1 ? h0 : h1;
    cfg.max_hop = h0 < h1 ? h1 : h0;
    cfg.max_channels = 1;
    cfg.max_frames = nframes;
    rc = pv_glide_create(&cfg, &a);
    if (rc != PV_OK) return fail("pv_glide_create", rc, NULL);
    rc = pv_glide_create(&cfg, &b);
    if (rc != PV_OK) return fail("pv_glide_create", rc, NULL);
    W = pv_vari_half_width(hs, cfg.min_hop, cfg.max_hop);
    hops = (int32_t *)malloc(sizeof(int32_t) * (size_t)nframes);
    if (!hops) return 1;
    for (m = 0; m < nframes; m++) {                        /* the linear ramp */
        hops[m] = (int32_t)floor((double)h0 + (double)(h1 - h0) * (double)m / (double)(nframes - 1) + 0.5);
        total += hops[m];
    }
    in = (float *)malloc(sizeof(float) * (size_t)total);
    out = (float *)malloc(sizeof(float) * (size_t)total);
    ref = (float *)malloc(sizeof(float) * (size_t)total);
    if (!in || !out || !ref) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    for (i = 0; i < total; i++) in[i] = (float)(0.5 * sin(2.0 * 3.14159265358979323846 * f0 * (double)i));
    rc = pv_glide_process(a, in, out, 1, nframes, hops, NULL, 0, total, total);
    if (rc != PV_OK) return fail("pv_glide_process", rc, a);
    for (m = 0; m < nframes; m += 3) {                     /* the same stream, three frames per call */
        const int nf = nframes - m < 3 ? nframes - m : 3;
        long n = 0;
        for (q = 0; q < nf; q++) n += hops[m + q];
        rc = pv_glide_process(b, in + done, ref + done, 1, nf, hops + m, NULL, 0, n, n);
        if (rc != PV_OK) return fail("pv_glide_process", rc, b);
        done += n;
    }
    same = done == total && memcmp(out, ref, sizeof(float) * (size_t)total) == 0;
    /* the first quarter of the frames, behind the stretch's onset of (ceil(N / hop) + 2) hs + N stretched samples, and the last quarter: the mean
     * pitch factor over frames [m0, m1) is sum hs / sum hop, and the content lags the curve by (N - hs) + W stretched samples, about that many
     * times hop / hs output samples */
    for (q = 0; q < 2; q++) {
        const int onset = (N + cfg.min_hop - 1) / cfg.min_hop + 2 + (N + hs - 1) / hs;
        const int m0 = q == 0 ? (onset < nframes / 4 - 1 ? onset : nframes / 4 - 1) : nframes - nframes / 4, m1 = q == 0 ? nframes / 4 : nframes;
        long at = 0;
        for (m = 0; m < m0; m++) at += hops[m];
        for (m = m0; m < m1; m++) sum[q] += hops[m];
        lag = (long)((double)(N - hs + W) * (double)sum[q] / ((double)(m1 - m0) * (double)hs));
        lo[q] = at + lag < total ? at + lag : total;
        hi[q] = at + sum[q] + lag < total ? at + sum[q] + lag : total;
        want[q] = (double)(m1 - m0) * (double)hs / (double)sum[q];
        got[q] = crossing_rate(out, lo[q], hi[q]) / f0;
    }
    printf("{\"frames\": %d, \"input_samples\": %ld, \"output_samples\": %ld, \"half_width\": %d, \"latency\": %d, "
           "\"pitch_factor_first\": %.6f, \"measured_pitch_factor_first\": %.6f, \"pitch_factor_last\": %.6f, \"measured_pitch_factor_last\": %.6f, "
           "\"one_call_equals_pieces\": %s}\n",
           nframes, total, done, (int)W, (int)(N - hs + W), want[0], got[0], want[1], got[1], same ? "true" : "false");
    pv_glide_destroy(a);
    pv_glide_destroy(b);
    free(hops);
    free(in);
    free(out);
    free(ref);
    return same ? 0 : 3;
}
