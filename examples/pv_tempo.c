/* pv_tempo.c -- variable tempo through the C ABI from plain C99: a tempo ramp on a generated tone, run once as one pv_tempo_process call and once
 * frame by frame on a second handle, and a JSON line that says whether the two outputs are the same bits.
 *
 *   cc -std=c99 -I include examples/pv_tempo.c -L phaze_amd/lib -lphaze_amd -lm -o pv_tempo
 *   ./pv_tempo [fft_size synthesis_hop min_hop max_hop nframes]      (default 1024 320 205 320 400: the analysis hop ramps from 205 to 320)
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
    const int hs = argc > 2 ? atoi(argv[2]) : 320;
    const int lo = argc > 3 ? atoi(argv[3]) : 205;
    const int hi = argc > 4 ? atoi(argv[4]) : 320;
    const int nframes = argc > 5 ? atoi(argv[5]) : 400;
    pv_stretch *a = NULL, *b = NULL;
    int32_t *hops;
    float *in, *out, *ref;
    double carry = 0.0, sum = 0.0;
    long i, nin = 0, nout, at = 0;
    int m, rc, same;
    if (nframes <= 0 || lo < 1 || hi < lo || hi > N) {
        fprintf(stderr, "need nframes > 0 and 1 <= min_hop <= max_hop <= fft_size\n");
        return 2;
    }
    /* the ramp: tempo (input samples per output sample) from lo / hs to hi / hs, turned into integer hops by error diffusion */
    hops = (int32_t *)malloc(sizeof(int32_t) * (size_t)nframes);
    if (!hops) return 1;
    for (m = 0; m < nframes; m++) {
        const double want = carry + lo + (double)(hi - lo) * m / (nframes > 1 ? nframes - 1 : 1);
        int h = (int)floor(want + 0.5);
        h = h < lo ? lo : h > hi ? hi : h;
        hops[m] = h;
        carry = want - h;
        nin += h;
    }
    cfg.fft_size = N;
    cfg.analysis_hop = lo;                                 /* the floor of the schedule */
    cfg.synthesis_hop = hs;
    cfg.max_channels = 1;
    cfg.max_frames = nframes;
    rc = pv_stretch_create(&cfg, &a);
    if (rc != PV_OK) return fail("pv_stretch_create", rc, NULL);
    rc = pv_stretch_create(&cfg, &b);
    if (rc != PV_OK) return fail("pv_stretch_create", rc, NULL);
    nout = (long)nframes * hs;
    in = (float *)malloc(sizeof(float) * (size_t)nin);
    out = (float *)malloc(sizeof(float) * (size_t)nout);
    ref = (float *)malloc(sizeof(float) * (size_t)nout);
    if (!in || !out || !ref) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    for (i = 0; i < nin; i++) in[i] = (float)(0.5 * sin(2.0 * 3.14159265358979323846 * 441.0 * (double)i / 48000.0));
    rc = pv_tempo_process(a, in, out, 1, nframes, hops, 0, nin, nout);
    if (rc != PV_OK) return fail("pv_tempo_process", rc, a);
    for (m = 0; m < nframes; m++) {                        /* the same schedule, one frame per call */
        rc = pv_tempo_process(b, in + at, ref + (long)m * hs, 1, 1, hops + m, 0, hops[m], hs);
        if (rc != PV_OK) return fail("pv_tempo_process", rc, b);
        at += hops[m];
    }
    same = memcmp(out, ref, sizeof(float) * (size_t)nout) == 0;
    for (i = N; i < nout; i++) sum += (double)out[i] * (double)out[i];      /* past the latency of N - hs samples */
    printf("{\"frames\": %d, \"input_samples\": %ld, \"output_samples\": %ld, \"min_hop\": %d, \"max_hop\": %d, \"output_rms\": %.6f, "
           "\"ramp_equals_frame_by_frame\": %s}\n",
           nframes, nin, nout, hops[0], hops[nframes - 1], nout > N ? sqrt(sum / (double)(nout - N)) : 0.0, same ? "true" : "false");
    pv_stretch_destroy(a);
    pv_stretch_destroy(b);
    free(hops);
    free(in);
    free(out);
    free(ref);
    return same ? 0 : 3;
}
