/* pv_contour.c -- pitch contour tracking through the C ABI from plain C99: a generated tone whose fundamental fades for a while is tracked both ways,
 * frame by frame (pv_f0_track) and as a path through eight candidates per frame (pv_contour_track, pv_contour_path); a JSON line with the number of
 * gross errors of each: voiced frames whose period is more than 20 % off the true one.  Where the fundamental is weak the dip at half the period falls
 * under the threshold first and pv_f0_track reads an octave up; the path stays on the period.
 *
 *   cc -std=c99 -I include examples/pv_contour.c -L phaze_amd/lib -lphaze_amd -lm -o pv_contour
 *   ./pv_contour [period_samples depth]      (default 217.3 0.97)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "phaze_amd.h"

#define WINDOW 512
#define MAX_LAG 512
#define MIN_LAG 32
#define HOP 128
#define K 8
#define N 12000

/* the voiced records more than 20 % off the period, and how many are unvoiced or empty */
static long gross(const int32_t *rec, long nrec, double period, long *unvoiced)
{
    long m, bad = 0;
    *unvoiced = 0;
    for (m = 0; m < nrec; m++) {
        const double p = pv_f0_period(rec + 4 * m);
        if (p <= 0.0) (*unvoiced)++;
        else if (fabs(p - period) > 0.2 * period) bad++;
    }
    return bad;
}

int main(int argc, char **argv)
{
    pv_f0_config fc = PV_F0_CONFIG_INIT;
    pv_contour_config cc = PV_CONTOUR_CONFIG_INIT;
    pv_contour_params cp = PV_CONTOUR_PARAMS_INIT;
    const double period = argc > 1 ? atof(argv[1]) : 217.3;
    const double depth = argc > 2 ? atof(argv[2]) : 0.97;
    const double two_pi = 2.0 * 3.14159265358979323846;
    const long nrec = (N - WINDOW - MAX_LAG) / HOP + 1;
    pv_f0 *f0 = NULL;
    pv_contour *ct = NULL;
    float *in;
    double *y, peak = 0.0;
    int32_t *rec, *cand, *path;
    uint32_t seed = 1u;
    long i, gross_f0, gross_path, unvoiced_f0, unvoiced_path;
    int rc;
    if (!(period >= 2.0 * MIN_LAG) || !(period < MAX_LAG - 1) || !(depth >= 0.0) || !(depth <= 1.0)) {
        fprintf(stderr, "need a period within [%d, %d) and a depth within [0, 1]\n", 2 * MIN_LAG, MAX_LAG - 1);
        return 2;
    }
    fc.window = WINDOW; fc.hop = HOP; fc.min_lag = MIN_LAG; fc.max_lag = MAX_LAG; fc.max_channels = 1;
    rc = pv_f0_create(&fc, &f0);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_create: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(NULL));
        return 1;
    }
    cc.window = WINDOW; cc.hop = HOP; cc.min_lag = MIN_LAG; cc.max_lag = MAX_LAG; cc.candidates = K; cc.max_channels = 1;
    rc = pv_contour_create(&cc, &ct);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_contour_create: %s (%s)\n", pv_status_string(rc), pv_contour_last_error(NULL));
        return 1;
    }
    in = (float *)malloc(sizeof(float) * N);
    y = (double *)malloc(sizeof(double) * N);
    rec = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    path = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    cand = (int32_t *)malloc(sizeof(int32_t) * 4 * K * (size_t)nrec);
    if (!in || !y || !rec || !path || !cand) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    for (i = 0; i < N; i++) {                              /* the fundamental fades by `depth` around samples 3000 and 9000; the octave stays; a little noise */
        const double a1 = 1.0 - depth * 0.5 * (1.0 - cos(two_pi * (double)i / 6000.0));
        const double ph = two_pi * (double)i / period;
        seed = seed * 1664525u + 1013904223u;
        y[i] = a1 * sin(ph) + 0.6 * sin(2.0 * ph + 0.3) + 0.04 * ((double)(seed >> 8) / 16777216.0 - 0.5);
        if (fabs(y[i]) > peak) peak = fabs(y[i]);
    }
    for (i = 0; i < N; i++) in[i] = (float)(0.8 * y[i] / peak);

    /* 1. frame by frame */
    rc = pv_f0_track(f0, in, 1, nrec, N, 2458, rec, nrec);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
        return 1;
    }
    gross_f0 = gross(rec, nrec, period, &unvoiced_f0);

    /* 2. eight candidates per frame, then the cheapest path through them: the same bias in both */
    rc = pv_contour_track(ct, in, 1, nrec, N, cp.bias, cand, nrec);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_contour_track: %s (%s)\n", pv_status_string(rc), pv_contour_last_error(ct));
        return 1;
    }
    cp.candidates = K; cp.max_lag = MAX_LAG;
    rc = pv_contour_path(&cp, cand, nrec, path, NULL);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_contour_path: %s\n", pv_status_string(rc));
        return 1;
    }
    gross_path = gross(path, nrec, period, &unvoiced_path);
    printf("{\"period\": %.3f, \"depth\": %.3f, \"frames\": %ld, \"gross_f0\": %ld, \"unvoiced_f0\": %ld, \"gross_contour\": %ld, \"unvoiced_contour\": %ld}\n",
           period, depth, nrec, gross_f0, unvoiced_f0, gross_path, unvoiced_path);
    pv_f0_destroy(f0);
    pv_contour_destroy(ct);
    free(in);
    free(y);
    free(rec);
    free(path);
    free(cand);
    return 0;
}
