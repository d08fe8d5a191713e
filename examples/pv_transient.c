/* pv_transient.c -- phase resets through the C ABI from plain C99: noise bursts over a tone, stretched so that the attacks pass unstretched.
 * pv_onset_strength counts rising bins per frame, pv_onsets_from_strength picks the onsets, pv_transient_plan writes the hop row and the reset row,
 * and pv_transient_process runs them -- once as one call and once frame by frame on a second handle.  A JSON line says whether the two outputs are the
 * same bits, how many onsets were found and how many frames were held.
 *
 *   cc -std=c99 -I include examples/pv_transient.c -L phaze_amd/lib -lphaze_amd -lm -o pv_transient
 *   ./pv_transient [fft_size nominal_hop synthesis_hop floor_hop nbursts]      (default 1024 256 384 192 3)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "phaze_amd.h"

static int fail(const char *what, int rc, const pv_stretch *h)
{
    fprintf(stderr, "%s: %s (%s)\n", what, pv_status_string(rc), pv_stretch_last_error(h));
    return 1;
}

int main(int argc, char **argv)
{
    pv_stretch_config cfg = PV_STRETCH_CONFIG_INIT;
    const int N = argc > 1 ? atoi(argv[1]) : 1024;
    const int ha = argc > 2 ? atoi(argv[2]) : 256;
    const int hs = argc > 3 ? atoi(argv[3]) : 384;
    const int fl = argc > 4 ? atoi(argv[4]) : 192;
    const int nbursts = argc > 5 ? atoi(argv[5]) : 3;
    pv_stretch *a = NULL, *b = NULL;
    int32_t *counts, *hops;
    uint8_t *resets;
    int64_t *onsets, nons, T, m, at = 0, held = 0;
    float *in, *out, *ref;
    double sum = 0.0;
    long i, n, nout;
    unsigned seed = 12345u;
    int k, rc, same, sframes;
    if (nbursts < 1 || fl < 1 || ha < fl || hs < fl) {
        fprintf(stderr, "need nbursts >= 1 and 1 <= floor_hop <= nominal_hop, floor_hop <= synthesis_hop\n");
        return 2;
    }
    n = (long)N * 10 * (nbursts + 1);
    sframes = (int)(n / fl);
    in = (float *)malloc(sizeof(float) * (size_t)n);
    counts = (int32_t *)malloc(sizeof(int32_t) * (size_t)sframes);
    if (!in || !counts) return 1;
    for (i = 0; i < n; i++) in[i] = (float)(0.1 * sin(2.0 * 3.14159265358979323846 * 0.0731 * (double)i));
    for (k = 1; k <= nbursts; k++) {                         /* a decaying noise burst every 10 N samples, off the frame grid */
        const long o = (long)N * 10 * k + 137 * k;
        for (i = 0; i < 1440 && o + i < n; i++) {
            seed = seed * 1664525u + 1013904223u;
            in[o + i] += (float)(((double)(seed >> 8) / 8388608.0 - 1.0) * exp(-(double)i / 120.0));
        }
    }
    cfg.fft_size = N;
    cfg.analysis_hop = fl;                                  /* the floor: every scheduled hop is >= it, and the strength's frames step by it */
    cfg.synthesis_hop = hs;
    cfg.max_channels = 1;
    cfg.max_frames = 64;
    if ((rc = pv_stretch_create(&cfg, &a)) != PV_OK) return fail("pv_stretch_create", rc, NULL);
    if ((rc = pv_stretch_create(&cfg, &b)) != PV_OK) return fail("pv_stretch_create", rc, NULL);
    /* strength -> onsets -> plan (two-call sizing: the first call counts) */
    if ((rc = pv_onset_strength(a, in, 1, sframes, n, counts, sframes)) != PV_OK) return fail("pv_onset_strength", rc, a);
    nons = pv_onsets_from_strength(counts, sframes, N, fl, 0.4, NULL, 0);
    if (nons < 0) return fail("pv_onsets_from_strength", (int)-nons, NULL);
    onsets = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nons > 0 ? nons : 1));
    if (!onsets) return 1;
    (void)pv_onsets_from_strength(counts, sframes, N, fl, 0.4, onsets, nons);
    T = pv_transient_plan(onsets, nons, n, N, ha, fl, hs, -1, -1, NULL, NULL, 0);      /* default lead N/8 and release N/2 */
    if (T <= 0) return fail("pv_transient_plan", T < 0 ? (int)-T : PV_ERR_ARGUMENT, NULL);
    hops = (int32_t *)malloc(sizeof(int32_t) * (size_t)T);
    resets = (uint8_t *)malloc((size_t)T);
    if (!hops || !resets) return 1;
    (void)pv_transient_plan(onsets, nons, n, N, ha, fl, hs, -1, -1, hops, resets, T);
    for (m = 0; m < T; m++) held += hops[m] == hs && hs != ha;
    nout = (long)T * hs;
    out = (float *)malloc(sizeof(float) * (size_t)nout);
    ref = (float *)malloc(sizeof(float) * (size_t)nout);
    if (!out || !ref) return 1;
    if ((rc = pv_transient_process(a, in, out, 1, (int32_t)T, hops, 0, resets, 0, n, nout)) != PV_OK) return fail("pv_transient_process", rc, a);
    for (m = 0; m < T; m++) {                                /* the same schedule one frame per call: the state carries the phases and the reset */
        if ((rc = pv_transient_process(b, in + at, ref + m * hs, 1, 1, hops + m, 0, resets + m, 0, hops[m], hs)) != PV_OK)
            return fail("pv_transient_process (frame by frame)", rc, b);
        at += hops[m];
    }
    same = memcmp(out, ref, sizeof(float) * (size_t)nout) == 0;
    for (i = 0; i < nout; i++) sum += (double)out[i] * out[i];
    printf("{\"fft_size\": %d, \"nominal_hop\": %d, \"synthesis_hop\": %d, \"floor_hop\": %d, \"frames\": %ld, \"onsets\": %ld, \"held_frames\": %ld, "
           "\"one_call_equals_frame_by_frame\": %s, \"output_rms\": %.6f}\n",
           N, ha, hs, fl, (long)T, (long)nons, (long)held, same ? "true" : "false", sqrt(sum / (double)nout));
    pv_stretch_destroy(a);
    pv_stretch_destroy(b);
    free(in); free(counts); free(onsets); free(hops); free(resets); free(out); free(ref);
    return same ? 0 : 3;
}
