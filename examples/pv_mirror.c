/* pv_mirror.c -- mirrored grains through the C ABI from plain C99: a generated signal, half a voiced tone and half white noise, is tracked (pv_f0_track)
 * and played at half speed twice, planned without and with mirrored grains (pv_mirror_plan, mirror = 0 and 1), through one pv_mirror handle
 * (pv_mirror_process), in one call and in three pieces cut at odd outputs.  At half speed every analysis mark of the noise serves two grains; played
 * forward twice the same grain repeats at the mark spacing and the noise buzzes at sample_rate / unvoiced_period, played once forward and once
 * backwards it does not.  A JSON line with the normalised autocorrelation of the noise part of either output at the lag unvoiced_period.
 * Exits non-zero unless the pieces equal the whole, bit for bit, and the mirrored figure is the lower one.
 *
 *   cc -std=c99 -I include examples/pv_mirror.c -L phaze_amd/lib -lphaze_amd -lm -o pv_mirror
 *   ./pv_mirror [frequency_hz seconds]      (default 220 1.0)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "phaze_amd.h"

#define RATE 48000.0
#define WINDOW 1024
#define MAX_LAG 1024
#define MIN_LAG 32
#define F0_HOP 256
#define MAX_PERIOD 1024
#define MAX_RATE 2
#define UNVOICED 128
#define PI 3.14159265358979323846

/* the normalised autocorrelation of x[lo, hi) at `lag`, about its mean */
static double autocorrelation(const float *x, long lo, long hi, long lag)
{
    double mean = 0.0, num = 0.0, den = 0.0;
    long i;
    for (i = lo; i < hi; i++) mean += x[i];
    mean /= (double)(hi - lo);
    for (i = lo; i < hi; i++) den += (x[i] - mean) * (x[i] - mean);
    for (i = lo; i + lag < hi; i++) num += (x[i] - mean) * (x[i + lag] - mean);
    return den > 0.0 ? num / den : 0.0;
}

int main(int argc, char **argv)
{
    pv_f0_config fc = PV_F0_CONFIG_INIT;
    pv_mirror_config mc = PV_MIRROR_CONFIG_INIT;
    pv_psola_params pp = PV_PSOLA_PARAMS_INIT;
    pv_epoch_params ep = PV_EPOCH_PARAMS_INIT;
    const double freq = argc > 1 ? atof(argv[1]) : 220.0;
    const double seconds = argc > 2 ? atof(argv[2]) : 1.0;
    const long n = (long)(seconds * RATE), half = n / 2;
    const long nrec = (n - WINDOW - MAX_LAG) / F0_HOP + 1;
    pv_f0 *f0 = NULL;
    pv_mirror *mh = NULL;
    float *in, *out[2], *pieces;
    int32_t *rec;
    double *rates, figure[2];
    uint32_t lcg = 12345u;
    long i, unvoiced = 0, mirrored[2] = {0, 0};
    int64_t ngrains[2], length[2];
    int rc, k, v, same = 1;
    if (!(freq > RATE / (MAX_LAG - 1)) || !(freq < RATE / MIN_LAG) || nrec < 40) {
        fprintf(stderr, "need a frequency the lags %d .. %d cover and at least %d samples\n", MIN_LAG, MAX_LAG - 1, WINDOW + MAX_LAG + 39 * F0_HOP);
        return 2;
    }
    fc.window = WINDOW; fc.hop = F0_HOP; fc.min_lag = MIN_LAG; fc.max_lag = MAX_LAG; fc.max_channels = 1;
    rc = pv_f0_create(&fc, &f0);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_create: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(NULL));
        return 1;
    }
    mc.max_period = MAX_PERIOD; mc.max_rate = MAX_RATE; mc.max_channels = 1; mc.max_outputs = 8192;
    rc = pv_mirror_create(&mc, &mh);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_mirror_create: %s (%s)\n", pv_status_string(rc), pv_mirror_last_error(NULL));
        return 1;
    }
    in = (float *)malloc(sizeof(float) * (size_t)n);
    out[0] = (float *)malloc(sizeof(float) * (size_t)(4 * n + 2 * MAX_PERIOD));
    out[1] = (float *)malloc(sizeof(float) * (size_t)(4 * n + 2 * MAX_PERIOD));
    pieces = (float *)malloc(sizeof(float) * (size_t)(4 * n + 2 * MAX_PERIOD));
    rec = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    rates = (double *)malloc(sizeof(double) * (size_t)nrec);
    if (!in || !out[0] || !out[1] || !pieces || !rec || !rates) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    /* six harmonics of `freq`, then white noise from a linear congruential generator */
    for (i = 0; i < half; i++) {
        double s = 0.0;
        for (k = 1; k <= 6; k++) s += cos(2.0 * PI * k * freq * (double)i / RATE + 0.7 * k) / (double)k;
        in[i] = (float)(0.3 * s);
    }
    for (i = half; i < n; i++) {
        lcg = lcg * 1664525u + 1013904223u;
        in[i] = (float)(0.2 * ((double)(lcg >> 8) / 8388608.0 - 1.0));
    }

    /* 1. estimate the fundamental per frame: the tone's records are voiced, the noise's are not */
    rc = pv_f0_track(f0, in, 1, nrec, n, 2458, rec, nrec);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
        return 1;
    }
    for (i = 0; i < nrec; i++) unvoiced += pv_f0_period(rec + 4 * i) > 0.0 ? 0 : 1;
    pp.f0_hop = F0_HOP; pp.f0_center = (WINDOW + MAX_LAG) / 2; pp.min_period = MIN_LAG; pp.max_period = MAX_PERIOD;
    pp.unvoiced_period = (double)UNVOICED; pp.input_len = n;
    for (i = 0; i < nrec; i++) rates[i] = 0.5;

    for (v = 0; v < 2; v++) {
        int32_t *grains;
        int64_t cut[4];
        /* 2. the grain table at half speed without (v = 0) and with (v = 1) mirrored grains, sized in two calls; the pitch is left alone */
        ngrains[v] = pv_mirror_plan(&pp, &ep, rec, nrec, NULL, rates, NULL, v, NULL, 0, &length[v]);
        if (ngrains[v] < 0 || length[v] > 4 * n + 2 * MAX_PERIOD) {
            fprintf(stderr, "pv_mirror_plan: bad argument\n");
            return 1;
        }
        grains = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(ngrains[v] > 0 ? ngrains[v] : 1));
        if (!grains) return 1;
        pv_mirror_plan(&pp, &ep, rec, nrec, NULL, rates, NULL, v, grains, ngrains[v], NULL);
        for (i = 0; i < (long)ngrains[v]; i++) mirrored[v] += (grains[4 * i + 1] >> 16) & 1;
        /* 3. overlap-add in one call, and in three pieces cut at odd outputs */
        rc = pv_mirror_process(mh, in, n, n, 1, grains, ngrains[v], out[v], 0, length[v], length[v]);
        cut[0] = 0; cut[1] = (length[v] / 3) | 1; cut[2] = (2 * length[v] / 3) | 1; cut[3] = length[v];
        for (k = 0; k < 3 && rc == PV_OK; k++)
            rc = pv_mirror_process(mh, in, n, n, 1, grains, ngrains[v], pieces + cut[k], cut[k], cut[k + 1] - cut[k], cut[k + 1] - cut[k]);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_mirror_process: %s (%s)\n", pv_status_string(rc), pv_mirror_last_error(mh));
            return 1;
        }
        free(grains);
        same = same && memcmp(pieces, out[v], sizeof(float) * (size_t)length[v]) == 0;
        /* the noise is the second half of the output: the middle of it */
        figure[v] = autocorrelation(out[v], 5 * (long)length[v] / 8, 7 * (long)length[v] / 8, UNVOICED);
    }
    printf("{\"frequency\": %.3f, \"samples\": %ld, \"records\": %ld, \"unvoiced_records\": %ld, \"unvoiced_period\": %d, "
           "\"forward\": {\"samples\": %ld, \"grains\": %ld, \"mirrored\": %ld, \"autocorrelation\": %.4f}, "
           "\"mirrored\": {\"samples\": %ld, \"grains\": %ld, \"mirrored\": %ld, \"autocorrelation\": %.4f}, \"pieces_equal_whole\": %s}\n",
           freq, n, nrec, unvoiced, UNVOICED, (long)length[0], (long)ngrains[0], mirrored[0], figure[0], (long)length[1], (long)ngrains[1], mirrored[1], figure[1],
           same ? "true" : "false");
    pv_f0_destroy(f0);
    pv_mirror_destroy(mh);
    free(in);
    free(out[0]);
    free(out[1]);
    free(pieces);
    free(rec);
    free(rates);
    if (!same) {
        fprintf(stderr, "the pieces differ from the whole\n");
        return 3;
    }
    if (!(figure[1] < figure[0]) || mirrored[0] != 0 || mirrored[1] == 0) {
        fprintf(stderr, "mirroring did not lower the autocorrelation at the mark spacing\n");
        return 4;
    }
    return 0;
}
