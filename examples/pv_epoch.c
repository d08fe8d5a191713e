/* pv_epoch.c -- epoch-aligned marks for the formant-preserving pitch correction, through the C ABI from plain C99: the two-formant, voice-like tone of
 * pv_psola.c, started half a period off the pulses, is tracked (pv_f0_track), the records become one period per frame (pv_epoch_periods) and the
 * epoch handle finds where in each frame the pulses sit (pv_epoch_track); the grain table is planned without the epoch records (pv_psola_plan) and with
 * them (pv_epoch_plan), and both tables are played (pv_psola_process).  A JSON line with the detected note, the corrected note either way (MIDI
 * numbers, 69 = A4), how many grains the records moved, and the strongest harmonic of the input and of both outputs (the first formant).
 *
 *   cc -std=c99 -I include examples/pv_epoch.c -L phaze_amd/lib -lphaze_amd -lm -o pv_epoch
 *   ./pv_epoch [frequency_hz seconds]      (default 452 1.0: a tone 47 cents above A4 = 440 Hz, brought down to it)
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
#define EPOCH_WINDOW 2048
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

/* the mean note over the voiced records [first, last) */
static double mean_note(const int32_t *rec, long first, long last)
{
    double sum = 0.0;
    long m, voiced = 0;
    for (m = first; m < last; m++) {
        const double p = pv_f0_period(rec + 4 * m);
        if (p > 0.0) {
            sum += 69.0 + 12.0 * log(RATE / p / 440.0) / log(2.0);
            voiced++;
        }
    }
    return voiced ? sum / (double)voiced : 0.0;
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
    pv_f0_config fc = PV_F0_CONFIG_INIT;
    pv_epoch_config ec = PV_EPOCH_CONFIG_INIT;
    pv_psola_config pc = PV_PSOLA_CONFIG_INIT;
    pv_tune_params tp = PV_TUNE_PARAMS_INIT;
    pv_psola_params pp = PV_PSOLA_PARAMS_INIT;
    pv_epoch_params ep = PV_EPOCH_PARAMS_INIT;
    const double freq = argc > 1 ? atof(argv[1]) : 452.0;
    const double seconds = argc > 2 ? atof(argv[2]) : 1.0;
    const long n = (long)(seconds * RATE);
    const long nrec = (n - WINDOW - MAX_LAG) / F0_HOP + 1;      /* EPOCH_WINDOW == WINDOW + MAX_LAG: as many epoch frames as f0 records */
    pv_f0 *f0 = NULL;
    pv_epoch *marks = NULL;
    pv_psola *ps = NULL;
    float *in, *out[2];
    int32_t *rec, *rec_out, *periods, *epochs, *grains[2];
    double *ratios, peak = 0.0, detected, corrected[2], note_hz, before, after[2];
    long i, found = 0, moved = 0;
    int64_t ngrains[2];
    int rc, k, v;
    if (!(freq > RATE / (MAX_LAG - 1)) || !(freq < RATE / MIN_LAG) || nrec < 8) {
        fprintf(stderr, "need a frequency the lags %d .. %d cover and at least %d samples\n", MIN_LAG, MAX_LAG - 1, WINDOW + MAX_LAG + 7 * F0_HOP);
        return 2;
    }
    fc.window = WINDOW; fc.hop = F0_HOP; fc.min_lag = MIN_LAG; fc.max_lag = MAX_LAG; fc.max_channels = 1;
    rc = pv_f0_create(&fc, &f0);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_create: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(NULL));
        return 1;
    }
    ec.window = EPOCH_WINDOW; ec.hop = F0_HOP; ec.max_period = MAX_PERIOD; ec.max_channels = 1;
    rc = pv_epoch_create(&ec, &marks);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_epoch_create: %s (%s)\n", pv_status_string(rc), pv_epoch_last_error(NULL));
        return 1;
    }
    pc.max_period = MAX_PERIOD; pc.max_channels = 1; pc.max_outputs = 8192;
    rc = pv_psola_create(&pc, &ps);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_psola_create: %s (%s)\n", pv_status_string(rc), pv_psola_last_error(NULL));
        return 1;
    }
    in = (float *)malloc(sizeof(float) * (size_t)n);
    out[0] = (float *)malloc(sizeof(float) * (size_t)n);
    out[1] = (float *)malloc(sizeof(float) * (size_t)n);
    rec = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    rec_out = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    periods = (int32_t *)malloc(sizeof(int32_t) * (size_t)nrec);
    epochs = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    ratios = (double *)malloc(sizeof(double) * (size_t)nrec);
    if (!in || !out[0] || !out[1] || !rec || !rec_out || !periods || !epochs || !ratios) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    /* a pulse train at `freq`, its first pulse half a period after sample 0, through the two resonators: the sum of its harmonics below 0.45 of the rate */
    memset(in, 0, sizeof(float) * (size_t)n);
    for (k = 1; k * freq < 0.45 * RATE; k++) {
        double mag, arg;
        formants(k * freq, &mag, &arg);
        for (i = 0; i < n; i++) in[i] += (float)(mag * cos(2.0 * PI * k * (freq * (double)i / RATE - 0.5) + arg));
    }
    for (i = 0; i < n; i++) peak = fabs((double)in[i]) > peak ? fabs((double)in[i]) : peak;
    for (i = 0; i < n; i++) in[i] = (float)(0.9 * (double)in[i] / peak);

    /* 1. the fundamental per frame, and from it the period row of the epoch handle */
    rc = pv_f0_track(f0, in, 1, nrec, n, 2458, rec, nrec);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
        return 1;
    }
    detected = mean_note(rec, 0, nrec);
    if (pv_epoch_periods(rec, nrec, periods, nrec) != nrec) {
        fprintf(stderr, "pv_epoch_periods: bad argument\n");
        return 1;
    }

    /* 2. where the pulses sit: one record per frame, at the tracker's hop on the same buffer */
    rc = pv_epoch_track(marks, in, 1, nrec, n, periods, epochs, nrec);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_epoch_track: %s (%s)\n", pv_status_string(rc), pv_epoch_last_error(marks));
        return 1;
    }
    for (i = 0; i < nrec; i++) found += epochs[4 * i + 1] > 0;

    /* 3. one ratio per record on the chromatic scale, then the grain table without (v = 0) and with (v = 1) the epoch records, sized in two calls */
    tp.sample_rate = RATE;
    if (pv_psola_ratios(&tp, rec, nrec, ratios, nrec) != nrec) {
        fprintf(stderr, "pv_psola_ratios: bad argument\n");
        return 1;
    }
    pp.f0_hop = F0_HOP; pp.f0_center = (WINDOW + MAX_LAG) / 2; pp.min_period = MIN_LAG; pp.max_period = MAX_PERIOD;
    pp.unvoiced_period = 256.0; pp.input_len = n;
    note_hz = 440.0 * pow(2.0, (floor(detected + 0.5) - 69.0) / 12.0);
    for (v = 0; v < 2; v++) {
        ngrains[v] = v ? pv_epoch_plan(&pp, &ep, rec, nrec, ratios, epochs, NULL, 0) : pv_psola_plan(&pp, rec, nrec, ratios, NULL, 0);
        if (ngrains[v] < 0) {
            fprintf(stderr, "%s: bad argument\n", v ? "pv_epoch_plan" : "pv_psola_plan");
            return 1;
        }
        grains[v] = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(ngrains[v] > 0 ? ngrains[v] : 1));
        if (!grains[v]) return 1;
        if (v) pv_epoch_plan(&pp, &ep, rec, nrec, ratios, epochs, grains[v], ngrains[v]);
        else pv_psola_plan(&pp, rec, nrec, ratios, grains[v], ngrains[v]);

        /* 4. overlap-add, and the result tracked the same way */
        rc = pv_psola_process(ps, in, n, n, 1, grains[v], ngrains[v], out[v], 0, n, n);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_psola_process: %s (%s)\n", pv_status_string(rc), pv_psola_last_error(ps));
            return 1;
        }
        rc = pv_f0_track(f0, out[v], 1, nrec, n, 2458, rec_out, nrec);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
            return 1;
        }
        corrected[v] = mean_note(rec_out, 4, nrec - 4);
        after[v] = strongest_harmonic(out[v], n / 4, 3 * n / 4, note_hz);
    }
    for (i = 0; i < ngrains[0] && i < ngrains[1]; i++) moved += grains[0][4 * i + 2] != grains[1][4 * i + 2];
    before = strongest_harmonic(in, n / 4, 3 * n / 4, freq);
    printf("{\"frequency\": %.3f, \"frames_tracked\": %ld, \"epochs_found\": %ld, \"detected_note\": %.4f, \"grains\": %ld, \"grains_moved\": %ld, "
           "\"corrected_note\": %.4f, \"corrected_note_epochs\": %.4f, \"strongest_harmonic_in\": %.1f, \"strongest_harmonic_out\": %.1f, "
           "\"strongest_harmonic_out_epochs\": %.1f}\n",
           freq, nrec, found, detected, (long)ngrains[1], moved, corrected[0], corrected[1], before, after[0], after[1]);
    pv_f0_destroy(f0);
    pv_epoch_destroy(marks);
    pv_psola_destroy(ps);
    free(in);
    free(out[0]);
    free(out[1]);
    free(rec);
    free(rec_out);
    free(periods);
    free(epochs);
    free(ratios);
    free(grains[0]);
    free(grains[1]);
    return 0;
}
