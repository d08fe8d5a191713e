/* pv_takes.c -- per-take plans through the C ABI from plain C99: three generated voice-like tones of different lengths and pitches (452 Hz, 223 Hz,
 * 331 Hz) are tracked (pv_f0_track), each is planned onto its nearest note at its own rate (1, 1/2, 2: pv_psola_ratios, pv_tsm_plan), and all three
 * are played by ONE pv_takes_process.  The same three plans then go through pv_tsm_process one by one, and the outputs are compared bit for bit.
 * Per take a line with the output's length and its note (MIDI numbers, 69 = A4), then `one_call_equals_three_tsm_calls 1`.
 *
 *   cc -std=c99 -I include examples/pv_takes.c -L phaze_amd/lib -lphaze_amd -lm -o pv_takes
 *   ./pv_takes
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
#define TAKES 3
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

/* a pulse train at `freq` through the two resonators, as the sum of its harmonics below 0.45 of the rate, peak 0.9 */
static void voice(float *x, long n, double freq)
{
    double peak = 0.0;
    long i;
    int k;
    memset(x, 0, sizeof(float) * (size_t)n);
    for (k = 1; k * freq < 0.45 * RATE; k++) {
        double mag, arg;
        formants(k * freq, &mag, &arg);
        for (i = 0; i < n; i++) x[i] += (float)(mag * cos(2.0 * PI * k * freq * (double)i / RATE + arg));
    }
    for (i = 0; i < n; i++) peak = fabs((double)x[i]) > peak ? fabs((double)x[i]) : peak;
    for (i = 0; i < n; i++) x[i] = (float)(0.9 * (double)x[i] / peak);
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

int main(void)
{
    static const double freq[TAKES] = {452.0, 223.0, 331.0}, seconds[TAKES] = {1.0, 0.7, 1.3}, speed[TAKES] = {1.0, 0.5, 2.0};
    pv_f0_config fc = PV_F0_CONFIG_INIT;
    pv_takes_config kc = PV_TAKES_CONFIG_INIT;
    pv_tsm_config tc = PV_TSM_CONFIG_INIT;
    pv_tune_params tp = PV_TUNE_PARAMS_INIT;
    pv_epoch_params ep = PV_EPOCH_PARAMS_INIT;
    pv_f0 *f0 = NULL;
    pv_takes *tk = NULL;
    pv_tsm *ts = NULL;
    pv_take take[TAKES];
    float *in[TAKES], *out[TAKES], *alone;
    int32_t *grains[TAKES], *rec, *rec_out;
    double *ratios, *rates, target[TAKES], note[TAKES];
    int64_t ngrains[TAKES], length[TAKES];
    long n[TAKES], voiced, i, longest = 0, most = 0;
    int rc, k, equal = 1;

    fc.window = WINDOW; fc.hop = F0_HOP; fc.min_lag = MIN_LAG; fc.max_lag = MAX_LAG; fc.max_channels = 1;
    rc = pv_f0_create(&fc, &f0);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_create: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(NULL));
        return 1;
    }
    kc.max_period = MAX_PERIOD; kc.max_rate = MAX_RATE; kc.max_channels = 1;
    rc = pv_takes_create(&kc, &tk);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_takes_create: %s (%s)\n", pv_status_string(rc), pv_takes_last_error(NULL));
        return 1;
    }
    tc.max_period = MAX_PERIOD; tc.max_rate = MAX_RATE; tc.max_channels = 1;
    rc = pv_tsm_create(&tc, &ts);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_tsm_create: %s (%s)\n", pv_status_string(rc), pv_tsm_last_error(NULL));
        return 1;
    }
    for (k = 0; k < TAKES; k++) {
        n[k] = (long)(seconds[k] * RATE);
        longest = n[k] > longest ? n[k] : longest;
    }
    rec = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(4 * longest / F0_HOP + 1));
    rec_out = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(4 * longest / F0_HOP + 1));
    ratios = (double *)malloc(sizeof(double) * (size_t)(longest / F0_HOP + 1));
    rates = (double *)malloc(sizeof(double) * (size_t)(longest / F0_HOP + 1));
    if (!rec || !rec_out || !ratios || !rates) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    tp.sample_rate = RATE;

    /* 1. per take: the tone, its f0 records, one ratio per record on the chromatic scale, and the grain table and output length at its own rate */
    for (k = 0; k < TAKES; k++) {
        pv_psola_params pp = PV_PSOLA_PARAMS_INIT;
        const long nrec = (n[k] - WINDOW - MAX_LAG) / F0_HOP + 1;
        in[k] = (float *)malloc(sizeof(float) * (size_t)n[k]);
        if (!in[k]) return 1;
        voice(in[k], n[k], freq[k]);
        rc = pv_f0_track(f0, in[k], 1, nrec, n[k], 2458, rec, nrec);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
            return 1;
        }
        target[k] = floor(mean_note(rec, 0, nrec, &voiced) + 0.5);
        if (pv_psola_ratios(&tp, rec, nrec, ratios, nrec) != nrec) {
            fprintf(stderr, "pv_psola_ratios: bad argument\n");
            return 1;
        }
        for (i = 0; i < nrec; i++) rates[i] = speed[k];
        pp.f0_hop = F0_HOP; pp.f0_center = (WINDOW + MAX_LAG) / 2; pp.min_period = MIN_LAG; pp.max_period = MAX_PERIOD;
        pp.unvoiced_period = 256.0; pp.input_len = n[k];
        ngrains[k] = pv_tsm_plan(&pp, &ep, rec, nrec, ratios, rates, NULL, NULL, 0, &length[k]);
        if (ngrains[k] < 0 || length[k] > 4 * n[k] + 2 * MAX_PERIOD) {
            fprintf(stderr, "pv_tsm_plan: bad argument\n");
            return 1;
        }
        grains[k] = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(ngrains[k] > 0 ? ngrains[k] : 1));
        out[k] = (float *)malloc(sizeof(float) * (size_t)(length[k] > 0 ? length[k] : 1));
        if (!grains[k] || !out[k]) return 1;
        pv_tsm_plan(&pp, &ep, rec, nrec, ratios, rates, NULL, grains[k], ngrains[k], NULL);
        take[k].in = in[k]; take[k].nin = n[k]; take[k].in_stride = n[k];
        take[k].grains = grains[k]; take[k].ngrains = ngrains[k];
        take[k].out = out[k]; take[k].out_first = 0; take[k].nout = length[k]; take[k].out_stride = length[k];
        most = (long)length[k] > most ? (long)length[k] : most;
    }

    /* 2. all three in one call */
    rc = pv_takes_process(tk, take, TAKES, 1);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_takes_process: %s (%s)\n", pv_status_string(rc), pv_takes_last_error(tk));
        return 1;
    }

    /* 3. each one alone through pv_tsm_process: the same bits; and the note of each output, tracked the same way */
    alone = (float *)malloc(sizeof(float) * (size_t)(most > 0 ? most : 1));
    if (!alone) return 1;
    for (k = 0; k < TAKES; k++) {
        const long nrec_out = ((long)length[k] - WINDOW - MAX_LAG) / F0_HOP + 1;
        rc = pv_tsm_process(ts, in[k], n[k], n[k], 1, grains[k], ngrains[k], alone, 0, length[k], length[k]);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_tsm_process: %s (%s)\n", pv_status_string(rc), pv_tsm_last_error(ts));
            return 1;
        }
        if (memcmp(alone, out[k], sizeof(float) * (size_t)length[k]) != 0) equal = 0;
        rc = pv_f0_track(f0, out[k], 1, nrec_out, length[k], 2458, rec_out, nrec_out);
        if (rc != PV_OK) {
            fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
            return 1;
        }
        note[k] = mean_note(rec_out, 4, nrec_out - 4, &voiced);
        printf("take %d frequency %.1f rate %.2f samples %ld output %ld grains %ld voiced %ld note %.4f target %.0f\n", k, freq[k], speed[k], n[k], (long)length[k],
               (long)ngrains[k], voiced, note[k], target[k]);
    }
    printf("one_call_equals_three_tsm_calls %d\n", equal);
    pv_f0_destroy(f0);
    pv_takes_destroy(tk);
    pv_tsm_destroy(ts);
    for (k = 0; k < TAKES; k++) {
        free(in[k]);
        free(out[k]);
        free(grains[k]);
    }
    free(alone);
    free(rec);
    free(rec_out);
    free(ratios);
    free(rates);
    return equal ? 0 : 1;
}
