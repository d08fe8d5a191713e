/* pv_formant.c -- formant shifting through the C ABI from plain C99: a generated two-formant, voice-like tone is tracked (pv_f0_track), the records become
 * one ratio each on the chromatic scale (pv_psola_ratios), and the tone is corrected onto the scale twice, with its formants moved up by 1.25 and down to
 * 0.8: one grain table per warp (pv_formant_plan) through one pv_formant handle (pv_formant_process), in one call and again in three pieces.  A JSON line
 * with, per warp, the output's note (MIDI numbers, 69 = A4) and its strongest harmonic (the first formant: it moves with the warp, whatever the note), and
 * whether the pieces equal the one call bit for bit.
 *
 *   cc -std=c99 -I include examples/pv_formant.c -L phaze_amd/lib -lphaze_amd -lm -o pv_formant
 *   ./pv_formant [frequency_hz seconds]      (default 452 1.0: a tone 47 cents above A4 = 440 Hz, brought down to it)
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

/* the mean note over the voiced records [first, last), and how many there were */
static double mean_note(const int32_t *rec, long first, long last, long *voiced)
{
    double sum = 0.0;
    long m;
    *voiced = 0;
    for (m = first; m < last; m++) {
        const double p = pv_f0_period(rec + 4 * m);
        if (p > 0.0) {
            sum += 69.0 + 12.0 * log(RATE / p / 440.0) / log(2.0);
            (*voiced)++;
        }
    }
    return *voiced ? sum / (double)*voiced : 0.0;
}

/* the frequency of the strongest harmonic of f0 below 5 kHz in x[lo, hi) */
static double strongest_harmonic(const float *x, long lo, long hi, double f0)
{
    double best = -1.0, best_hz = 0.0;
    int k;
    for (k = 1; k * f0 < 5000.0; k++) {
        const double w = 2.0 * PI * k * f0 / RATE;
        double re = 0.0, im = 0.0;
        long i;
        for (i = lo; i < hi; i++) {
            re += x[i] * cos(w * (double)i);
            im += x[i] * sin(w * (double)i);
        }
        if (re * re + im * im > best) {
            best = re * re + im * im;
            best_hz = k * f0;
        }
    }
    return best_hz;
}

int main(int argc, char **argv)
{
    static const double warp[2] = {1.25, 0.8};
    pv_f0_config fc = PV_F0_CONFIG_INIT;
    pv_formant_config tc = PV_FORMANT_CONFIG_INIT;
    pv_tune_params tp = PV_TUNE_PARAMS_INIT;
    pv_psola_params pp = PV_PSOLA_PARAMS_INIT;
    pv_epoch_params ep = PV_EPOCH_PARAMS_INIT;
    const double freq = argc > 1 ? atof(argv[1]) : 452.0;
    const double seconds = argc > 2 ? atof(argv[2]) : 1.0;
    const long n = (long)(seconds * RATE);
    const long nrec = (n - WINDOW - MAX_LAG) / F0_HOP + 1;
    pv_f0 *f0 = NULL;
    pv_formant *fm = NULL;
    float *in, *out, *pieces;
    int32_t *rec, *rec_out;
    double *ratios, *warps, peak = 0.0, detected, note_hz, before, note[2], after[2];
    long i, voiced_in, voiced_out[2], warped[2];
    int64_t ngrains[2], length[2];
    int rc, k, v, equal = 1;
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
    tc.max_period = MAX_PERIOD; tc.max_rate = MAX_RATE; tc.max_channels = 1; tc.max_outputs = 8192;
    rc = pv_formant_create(&tc, &fm);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_formant_create: %s (%s)\n", pv_status_string(rc), pv_formant_last_error(NULL));
        return 1;
    }
    in = (float *)malloc(sizeof(float) * (size_t)n);
    out = (float *)malloc(sizeof(float) * (size_t)(n + 2 * MAX_PERIOD));
    pieces = (float *)malloc(sizeof(float) * (size_t)(n + 2 * MAX_PERIOD));
    rec = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    rec_out = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(nrec + 16));
    ratios = (double *)malloc(sizeof(double) * (size_t)nrec);
    warps = (double *)malloc(sizeof(double) * (size_t)nrec);
    if (!in || !out || !pieces || !rec || !rec_out || !ratios || !warps) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    /* a pulse train at `freq` through the two resonators, as the sum of its harmonics below 0.45 of the rate */
    memset(in, 0, sizeof(float) * (size_t)n);
    for (k = 1; k * freq < 0.45 * RATE; k++) {
        double mag, arg;
        formants(k * freq, &mag, &arg);
        for (i = 0; i < n; i++) in[i] += (float)(mag * cos(2.0 * PI * k * freq * (double)i / RATE + arg));
    }
    for (i = 0; i < n; i++) peak = fabs((double)in[i]) > peak ? fabs((double)in[i]) : peak;
    for (i = 0; i < n; i++) in[i] = (float)(0.9 * (double)in[i] / peak);

    /* 1. estimate the fundamental per frame, and one ratio per record on the chromatic scale */
    rc = pv_f0_track(f0, in, 1, nrec, n, 2458, rec, nrec);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
        return 1;
    }
    detected = mean_note(rec, 0, nrec, &voiced_in);
    note_hz = 440.0 * pow(2.0, (floor(detected + 0.5) - 69.0) / 12.0);
    before = strongest_harmonic(in, n / 4, 3 * n / 4, freq);
    tp.sample_rate = RATE;
    if (pv_psola_ratios(&tp, rec, nrec, ratios, nrec) != nrec) {
        fprintf(stderr, "pv_psola_ratios: bad argument\n");
        return 1;
    }
    pp.f0_hop = F0_HOP; pp.f0_center = (WINDOW + MAX_LAG) / 2; pp.min_period = MIN_LAG; pp.max_period = MAX_PERIOD;
    pp.unvoiced_period = 256.0; pp.input_len = n;

    for (v = 0; v < 2; v++) {
        int32_t *grains;
        long nrec_out;
        int64_t cut[4];
        /* 2. the grain table at this warp, sized in two calls (rates NULL: the output is as long as the input) */
        for (i = 0; i < nrec; i++) warps[i] = warp[v];
        ngrains[v] = pv_formant_plan(&pp, &ep, rec, nrec, ratios, NULL, warps, NULL, NULL, 0, &length[v]);
        if (ngrains[v] < 0 || length[v] > n + 2 * MAX_PERIOD) {
            fprintf(stderr, "pv_formant_plan: bad argument\n");
            return 1;
        }
        grains = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(ngrains[v] > 0 ? ngrains[v] : 1));
        if (!grains) return 1;
        pv_formant_plan(&pp, &ep, rec, nrec, ratios, NULL, warps, NULL, grains, ngrains[v], NULL);
        warped[v] = 0;
        for (i = 0; i < (long)ngrains[v]; i++) warped[v] += (grains[4 * i + 1] >> 17) != 0;
        /* 3. overlap-add in one call, and again in three pieces cut at odd outputs */
        rc = pv_formant_process(fm, in, n, n, 1, grains, ngrains[v], out, 0, length[v], length[v]);
        cut[0] = 0; cut[1] = length[v] / 3 + 1; cut[2] = 2 * length[v] / 3 + 5; cut[3] = length[v];
        for (k = 0; k < 3 && rc == PV_OK; k++)
            rc = pv_formant_process(fm, in, n, n, 1, grains, ngrains[v], pieces + cut[k], cut[k], cut[k + 1] - cut[k], cut[k + 1] - cut[k]);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_formant_process: %s (%s)\n", pv_status_string(rc), pv_formant_last_error(fm));
            return 1;
        }
        equal = equal && memcmp(out, pieces, sizeof(float) * (size_t)length[v]) == 0;
        free(grains);
        /* the result, tracked the same way */
        nrec_out = ((long)length[v] - WINDOW - MAX_LAG) / F0_HOP + 1;
        rc = pv_f0_track(f0, out, 1, nrec_out, length[v], 2458, rec_out, nrec_out);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
            return 1;
        }
        note[v] = mean_note(rec_out, 4, nrec_out - 4, &voiced_out[v]);
        after[v] = strongest_harmonic(out, (long)length[v] / 4, 3 * (long)length[v] / 4, note_hz);
    }
    printf("{\"frequency\": %.3f, \"samples\": %ld, \"detected_note\": %.4f, \"strongest_harmonic_in\": %.1f, "
           "\"up\": {\"warp\": %.2f, \"samples\": %ld, \"grains\": %ld, \"warped\": %ld, \"voiced\": %ld, \"note\": %.4f, \"strongest_harmonic\": %.1f}, "
           "\"down\": {\"warp\": %.2f, \"samples\": %ld, \"grains\": %ld, \"warped\": %ld, \"voiced\": %ld, \"note\": %.4f, \"strongest_harmonic\": %.1f}, "
           "\"one_call_equals_pieces\": %s}\n",
           freq, n, detected, before, warp[0], (long)length[0], (long)ngrains[0], warped[0], voiced_out[0], note[0], after[0], warp[1], (long)length[1], (long)ngrains[1],
           warped[1], voiced_out[1], note[1], after[1], equal ? "true" : "false");
    pv_f0_destroy(f0);
    pv_formant_destroy(fm);
    free(in);
    free(out);
    free(pieces);
    free(rec);
    free(rec_out);
    free(ratios);
    free(warps);
    return equal ? 0 : 1;
}
