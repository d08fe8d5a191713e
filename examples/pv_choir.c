/* pv_choir.c -- full-grain harmony voices through the C ABI from plain C99: a generated two-formant, voice-like tone near A3 that ends in a stretch of
 * noise is tracked (pv_f0_track), the records become one row of ratios per voice in C major (pv_harmony_ratios: the lead corrected onto the scale and a
 * third below it), every voice gets its own grain table at half tempo (pv_choir_plan, rate 1/2, mirror = 1: in the noise every second use of a mark plays
 * backwards, so the slowed noise does not buzz), the lead at warp 1 and the third below at warp 0.85 (its formants lowered: a different singer, not a
 * slowed-down tape), and one pv_choir handle overlap-adds and sums the two in one call (pv_choir_process).  The same output in three calls split at odd
 * positions is the same bit for bit.  A JSON line with the output's length, the notes and the level of the output at their fundamentals.
 *
 *   cc -std=c99 -I include examples/pv_choir.c -L phaze_amd/lib -lphaze_amd -lm -o pv_choir
 *   ./pv_choir [frequency_hz seconds]      (default 223 1.0: a tone 23 cents above A3 = 220 Hz; the voices land on A3 and on F3 below it)
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
#define VOICES 2
#define C_MAJOR 0xAB5 /* C D E F G A B */
#define PI 3.14159265358979323846

/* magnitude and phase of the two resonators (1200 and 2600 Hz) in cascade at `hz` */
static void formants(double hz, double *mag, double *arg)
{
    static const double centre[2] = {1200.0, 2600.0}, width[2] = {80.0, 120.0};
    const double w = 2.0 * PI * hz / RATE;
    int k;
    *mag = 1.0;
    *arg = 0.0;
    for (k = 0; k < 2; k++) {
        const double r = exp(-PI * width[k] / RATE), c = 2.0 * r * cos(2.0 * PI * centre[k] / RATE);
        const double re = 1.0 - c * cos(w) + r * r * cos(2.0 * w), im = c * sin(w) - r * r * sin(2.0 * w);
        *mag /= sqrt(re * re + im * im);
        *arg -= atan2(im, re);
    }
}

/* the amplitude of x[lo, hi) at `hz` */
static double level(const float *x, long lo, long hi, double hz)
{
    const double w = 2.0 * PI * hz / RATE;
    double re = 0.0, im = 0.0;
    long i;
    for (i = lo; i < hi; i++) {
        re += x[i] * cos(w * (double)i);
        im += x[i] * sin(w * (double)i);
    }
    return 2.0 * sqrt(re * re + im * im) / (double)(hi - lo);
}

int main(int argc, char **argv)
{
    static const int32_t degrees[VOICES] = {0, -2};
    static const double warp[VOICES] = {1.0, 0.85};
    static const float gains[VOICES] = {0.6f, 0.4f};
    pv_f0_config fc = PV_F0_CONFIG_INIT;
    pv_choir_config hc = PV_CHOIR_CONFIG_INIT;
    pv_tune_params tp = PV_TUNE_PARAMS_INIT;
    pv_psola_params pp = PV_PSOLA_PARAMS_INIT;
    pv_epoch_params ep = PV_EPOCH_PARAMS_INIT;
    const double freq = argc > 1 ? atof(argv[1]) : 223.0;
    const double seconds = argc > 2 ? atof(argv[2]) : 1.0;
    const long n = (long)(seconds * RATE);
    const long nrec = (n - WINDOW - MAX_LAG) / F0_HOP + 1;
    pv_f0 *f0 = NULL;
    pv_choir *hv = NULL;
    float *in, *out, *pieces;
    int32_t *rec, *grains;
    double *ratios, *rates, *warps, peak = 0.0, note_hz[VOICES], found[VOICES], mean[VOICES];
    int64_t voice_first[VOICES + 1], count[VOICES], length[VOICES], cut[4], mirrored = 0, both = 0;
    const long voiced = 3 * n / 5;
    unsigned long seed = 12345UL;
    long i;
    int rc, k, v, same;
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
    hc.max_period = MAX_PERIOD; hc.max_rate = MAX_RATE; hc.max_voices = VOICES; hc.max_channels = 1; hc.max_outputs = 8192;
    rc = pv_choir_create(&hc, &hv);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_choir_create: %s (%s)\n", pv_status_string(rc), pv_choir_last_error(NULL));
        return 1;
    }
    in = (float *)malloc(sizeof(float) * (size_t)n);
    out = (float *)malloc(sizeof(float) * (size_t)(2 * n + 2 * MAX_PERIOD));
    pieces = (float *)malloc(sizeof(float) * (size_t)(2 * n + 2 * MAX_PERIOD));
    rec = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    ratios = (double *)malloc(sizeof(double) * VOICES * (size_t)nrec);
    rates = (double *)malloc(sizeof(double) * (size_t)nrec);
    warps = (double *)malloc(sizeof(double) * (size_t)nrec);
    if (!in || !out || !pieces || !rec || !ratios || !rates || !warps) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    /* a pulse train at `freq` through the two resonators, as the sum of its harmonics below 0.45 of the rate, for the first three fifths; then noise */
    memset(in, 0, sizeof(float) * (size_t)n);
    for (k = 1; k * freq < 0.45 * RATE; k++) {
        double mag, arg;
        formants(k * freq, &mag, &arg);
        for (i = 0; i < voiced; i++) in[i] += (float)(mag * cos(2.0 * PI * k * freq * (double)i / RATE + arg));
    }
    for (i = 0; i < n; i++) peak = fabs((double)in[i]) > peak ? fabs((double)in[i]) : peak;
    for (i = 0; i < voiced; i++) in[i] = (float)(0.9 * (double)in[i] / peak);
    for (i = voiced; i < n; i++) {
        seed = (seed * 1103515245UL + 12345UL) & 0x7fffffffUL;
        in[i] = (float)(0.2 * ((double)seed / 1073741824.0 - 1.0));
    }

    /* 1. estimate the fundamental per frame, and one row of ratios per voice: the lead onto C major and a third below it */
    rc = pv_f0_track(f0, in, 1, nrec, n, 2458, rec, nrec);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
        return 1;
    }
    tp.sample_rate = RATE; tp.scale_mask = C_MAJOR;
    if (pv_harmony_ratios(&tp, rec, nrec, degrees, VOICES, ratios, nrec) != nrec) {
        fprintf(stderr, "pv_harmony_ratios: bad argument\n");
        return 1;
    }
    for (v = 0; v < VOICES; v++) {
        mean[v] = 0.0;
        for (i = 4; i < nrec / 2; i++) mean[v] += ratios[v * nrec + i] / (double)(nrec / 2 - 4);
        note_hz[v] = freq * mean[v];
    }

    /* 2. one grain table per voice on the same time base (rate 1/2, mirrored reuses), each at its own warp, sized in two calls and laid one after the other */
    pp.f0_hop = F0_HOP; pp.f0_center = (WINDOW + MAX_LAG) / 2; pp.min_period = MIN_LAG; pp.max_period = MAX_PERIOD;
    pp.unvoiced_period = 256.0; pp.input_len = n;
    voice_first[0] = 0;
    for (i = 0; i < nrec; i++) rates[i] = 0.5;
    for (v = 0; v < VOICES; v++) {
        for (i = 0; i < nrec; i++) warps[i] = warp[v];
        count[v] = pv_choir_plan(&pp, &ep, rec, nrec, ratios + v * nrec, rates, warps, NULL, 1, NULL, 0, &length[v]);
        if (count[v] < 0 || length[v] > 2 * n + 2 * MAX_PERIOD) {
            fprintf(stderr, "pv_choir_plan: bad argument\n");
            return 1;
        }
        voice_first[v + 1] = voice_first[v] + count[v];
    }
    grains = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(voice_first[VOICES] > 0 ? voice_first[VOICES] : 1));
    if (!grains) return 1;
    for (v = 0; v < VOICES; v++) {
        for (i = 0; i < nrec; i++) warps[i] = warp[v];
        pv_choir_plan(&pp, &ep, rec, nrec, ratios + v * nrec, rates, warps, NULL, 1, grains + 4 * voice_first[v], count[v], NULL);
    }
    for (i = 0; i < voice_first[VOICES]; i++) {
        const int32_t w = grains[4 * i + 1];
        mirrored += (w >> 16) & 1;
        both += ((w >> 16) & 1) && (w >> 17) != 0;
    }

    /* 3. overlap-add every voice and sum them: one call */
    rc = pv_choir_process(hv, in, n, n, 1, grains, voice_first, VOICES, gains, out, 0, length[0], length[0]);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_choir_process: %s (%s)\n", pv_status_string(rc), pv_choir_last_error(hv));
        return 1;
    }
    /* the same in three pieces split at odd positions: the order of every sum depends on (voice, grain, tap) alone */
    cut[0] = 0; cut[1] = length[0] / 3 + 1; cut[2] = 2 * length[0] / 3 + 7; cut[3] = length[0];
    for (k = 0; k < 3; k++) {
        rc = pv_choir_process(hv, in, n, n, 1, grains, voice_first, VOICES, gains, pieces + cut[k], cut[k], cut[k + 1] - cut[k], cut[k + 1] - cut[k]);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_choir_process: %s (%s)\n", pv_status_string(rc), pv_choir_last_error(hv));
            return 1;
        }
    }
    same = memcmp(out, pieces, sizeof(float) * (size_t)length[0]) == 0;
    /* the voiced part of the output: the first three fifths, at half tempo */
    for (v = 0; v < VOICES; v++) found[v] = level(out, (long)length[0] / 10, (long)length[0] / 2, note_hz[v]);
    printf("{\"frequency\": %.3f, \"samples\": %ld, \"output_samples\": %ld, \"grains\": [%ld, %ld], \"mirrored\": %ld, \"mirrored_and_warped\": %ld, "
           "\"ratios\": [%.6f, %.6f], \"note_hz\": [%.3f, %.3f], \"level\": [%.5f, %.5f], \"level_in_at_third_below\": %.5f, "
           "\"one_call_equals_three_pieces\": %s}\n",
           freq, n, (long)length[0], (long)count[0], (long)count[1], (long)mirrored, (long)both, mean[0], mean[1], note_hz[0], note_hz[1], found[0], found[1],
           level(in, n / 10, voiced - n / 10, note_hz[1]), same ? "true" : "false");
    pv_f0_destroy(f0);
    pv_choir_destroy(hv);
    free(pieces);
    free(rates);
    free(warps);
    free(in);
    free(out);
    free(rec);
    free(ratios);
    free(grains);
    return same ? 0 : 1;
}
