/* pv_stretch.c -- the time-stretch C ABI from plain C99: stretch a generated tone and print the output length and RMS.
 *
 *   cc -std=c99 -I include examples/pv_stretch.c -L phaze_amd/lib -lphaze_amd -lm -o pv_stretch
 *   ./pv_stretch [fft_size analysis_hop synthesis_hop nframes]      (default 1024 256 320 400: 1.25x longer, same pitch)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "phaze_amd.h"

int main(int argc, char **argv)
{
    pv_stretch_config cfg = PV_STRETCH_CONFIG_INIT;
    const int nframes = argc > 4 ? atoi(argv[4]) : 400;
    pv_stretch *h = NULL;
    float *in, *out;
    double sum = 0.0;
    long i, nin, nout;
    int rc;
    cfg.fft_size = argc > 1 ? atoi(argv[1]) : 1024;
    cfg.analysis_hop = argc > 2 ? atoi(argv[2]) : 256;
    cfg.synthesis_hop = argc > 3 ? atoi(argv[3]) : 320;
    cfg.max_channels = 1;
    cfg.max_frames = nframes;
    if (nframes <= 0) {
        fprintf(stderr, "nframes must be positive\n");
        return 2;
    }
    rc = pv_stretch_create(&cfg, &h);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_stretch_create: %s (%s)\n", pv_status_string(rc), pv_stretch_last_error(NULL));
        return 1;
    }
    nin = (long)nframes * cfg.analysis_hop;
    nout = (long)nframes * cfg.synthesis_hop;
    in = (float *)malloc(sizeof(float) * (size_t)nin);
    out = (float *)malloc(sizeof(float) * (size_t)nout);
    if (!in || !out) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    for (i = 0; i < nin; i++) in[i] = (float)(0.5 * sin(2.0 * 3.14159265358979323846 * 441.0 * (double)i / 48000.0));
    rc = pv_stretch_process(h, in, out, 1, nframes, nin, nout);
    if (rc != PV_OK) {
        fprintf(stderr, "pv_stretch_process: %s (%s)\n", pv_status_string(rc), pv_stretch_last_error(h));
        return 1;
    }
    for (i = cfg.fft_size; i < nout; i++) sum += (double)out[i] * (double)out[i];      /* past the latency of N - hs samples */
    printf("{\"input_samples\": %ld, \"output_samples\": %ld, \"output_rms\": %.6f}\n", nin, nout,
           nout > cfg.fft_size ? sqrt(sum / (double)(nout - cfg.fft_size)) : 0.0);
    pv_stretch_destroy(h);
    free(in);
    free(out);
    return 0;
}
