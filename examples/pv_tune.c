/* pv_tune.c -- pitch correction through the C ABI from plain C99: a generated, detuned tone is tracked (pv_f0_track), the records are planned onto
 * the chromatic scale (pv_tune_plan), the plan is played through a pv_glide handle (pv_glide_process) and the result is tracked again; a JSON line
 * with the detected and the corrected note (MIDI numbers, 69 = A4) and the mean planned hop.
 *
 *   cc -std=c99 -I include examples/pv_tune.c -L phaze_amd/lib -lphaze_amd -lm -o pv_tune
 *   ./pv_tune [frequency_hz seconds]      (default 452 1.0: a tone 47 cents above A4 = 440 Hz, brought down to it)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "phaze_amd.h"

#define RATE 48000.0
#define WINDOW 1024
#define MAX_LAG 1024
#define F0_HOP 256
#define FFT_SIZE 1024
#define SYNTHESIS_HOP 256
#define MIN_HOP 128
#define MAX_HOP 512

/* the mean note over the voiced records [first, nrec), and how many there were */
static double mean_note(const int32_t *rec, long first, long nrec, long *voiced)
{
    double sum = 0.0;
    long m;
    *voiced = 0;
    for (m = first; m < nrec; m++) {
        const double p = pv_f0_period(rec + 4 * m);
        if (p > 0.0) {
            sum += 69.0 + 12.0 * log(RATE / p / 440.0) / log(2.0);
            (*voiced)++;
        }
    }
    return *voiced ? sum / (double)*voiced : 0.0;
}

int main(int argc, char **argv)
{
    pv_f0_config fc = PV_F0_CONFIG_INIT;
    pv_glide_config gc = PV_GLIDE_CONFIG_INIT;
    pv_tune_params tp = PV_TUNE_PARAMS_INIT;
    const double freq = argc > 1 ? atof(argv[1]) : 452.0;
    const double seconds = argc > 2 ? atof(argv[2]) : 1.0;
    const long n = (long)(seconds * RATE);
    const long nrec = (n - WINDOW - MAX_LAG) / F0_HOP + 1;
    pv_f0 *f0 = NULL;
    pv_glide *glide = NULL;
    float *in, *out;
    int32_t *rec, *rec_out, *hops;
    long i, total = 0, nrec_out, skip, voiced_in, voiced_out;
    int64_t nhops, m;
    int32_t W;
    double detected, corrected;
    int rc;
    if (!(freq > RATE / (MAX_LAG - 1)) || !(freq < RATE / 32.0) || nrec < 8) {
        fprintf(stderr, "need a frequency the lags 32 .. %d cover and at least %d samples\n", MAX_LAG - 1, WINDOW + MAX_LAG + 7 * F0_HOP);
        return 2;
    }
    fc.window = WINDOW; fc.hop = F0_HOP; fc.min_lag = 32; fc.max_lag = MAX_LAG; fc.max_channels = 1;
    rc = pv_f0_create(&fc, &f0);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_create: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(NULL));
        return 1;
    }
    gc.fft_size = FFT_SIZE; gc.synthesis_hop = SYNTHESIS_HOP; gc.min_hop = MIN_HOP; gc.max_hop = MAX_HOP; gc.max_channels = 1;
    rc = pv_glide_create(&gc, &glide);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_glide_create: %s (%s)\n", pv_status_string(rc), pv_glide_last_error(NULL));
        return 1;
    }
    in = (float *)malloc(sizeof(float) * (size_t)n);
    out = (float *)malloc(sizeof(float) * (size_t)n);
    rec = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    rec_out = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nrec);
    if (!in || !out || !rec || !rec_out) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    for (i = 0; i < n; i++) {                              /* the fundamental and its octave */
        const double ph = 2.0 * 3.14159265358979323846 * freq * (double)i / RATE;
        in[i] = (float)(0.5 * sin(ph) + 0.25 * sin(2.0 * ph));
    }

    /* 1. estimate the fundamental per frame */
    rc = pv_f0_track(f0, in, 1, nrec, n, 2458, rec, nrec);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
        return 1;
    }
    detected = mean_note(rec, 0, nrec, &voiced_in);

    /* 2. snap it to the scale: the plan of hops, sized in two calls.  The glide's curve acts at output time, (N - hs) + W stretched samples behind the
     * content: the plan looks that far ahead (about as many input samples, the hops staying near the synthesis hop) */
    W = pv_vari_half_width(SYNTHESIS_HOP, MIN_HOP, MAX_HOP);
    tp.f0_hop = F0_HOP; tp.f0_center = (WINDOW + MAX_LAG) / 2; tp.sample_rate = RATE;
    tp.synthesis_hop = SYNTHESIS_HOP; tp.min_hop = MIN_HOP; tp.max_hop = MAX_HOP;
    tp.input_len = n; tp.shift = -(FFT_SIZE - SYNTHESIS_HOP + W);
    nhops = pv_tune_plan(&tp, rec, nrec, NULL, NULL, 0);
    if (nhops < 0) {
        fprintf(stderr, "pv_tune_plan: bad argument\n");
        return 1;
    }
    hops = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nhops > 0 ? nhops : 1));
    if (!hops) return 1;
    pv_tune_plan(&tp, rec, nrec, hops, NULL, nhops);
    for (m = 0; m < nhops; m++) total += hops[m];

    /* 3. glide there */
    rc = pv_glide_process(glide, in, out, 1, (int32_t)nhops, hops, NULL, 0, total, total);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_glide_process: %s (%s)\n", pv_status_string(rc), pv_glide_last_error(glide));
        return 1;
    }

    /* the result, tracked the same way, behind the stretch's onset */
    nrec_out = (total - WINDOW - MAX_LAG) / F0_HOP + 1;
    rc = pv_f0_track(f0, out, 1, nrec_out, total, 2458, rec_out, nrec_out);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_f0_track: %s (%s)\n", pv_status_string(rc), pv_f0_last_error(f0));
        return 1;
    }
    skip = (2 * FFT_SIZE + W) / F0_HOP + 1;
    corrected = mean_note(rec_out, skip < nrec_out ? skip : nrec_out, nrec_out, &voiced_out);
    printf("{\"frequency\": %.3f, \"frames_tracked\": %ld, \"voiced\": %ld, \"detected_note\": %.4f, \"frames_planned\": %ld, \"mean_hop\": %.4f, "
           "\"output_samples\": %ld, \"voiced_out\": %ld, \"corrected_note\": %.4f}\n",
           freq, nrec, voiced_in, detected, (long)nhops, nhops ? (double)total / (double)nhops : 0.0, total, voiced_out, corrected);
    pv_f0_destroy(f0);
    pv_glide_destroy(glide);
    free(in);
    free(out);
    free(rec);
    free(rec_out);
    free(hops);
    return 0;
}
