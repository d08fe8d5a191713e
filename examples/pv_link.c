/* pv_link.c -- linked channels through the C ABI from plain C99: a stereo tone whose right channel leads the left by 90 degrees, stretched by
 * synthesis_hop / analysis_hop once on a linked handle (pv_link_channels(h, 2): one phase track for the pair) and once on an unlinked one, and the
 * output phase offset between the channels of each, fitted by least squares over the steady part of the output.
 *
 *   cc -std=c99 -I include examples/pv_link.c -L phaze_amd/lib -lphaze_amd -lm -o pv_link
 *   ./pv_link [fft_size analysis_hop synthesis_hop nframes]      (default 1024 205 256 400: a 1.25x stretch)
 *
 * Prints "linked offset deg: ..." (90 up to rounding) and "unlinked offset deg: ..." (each channel's phase is scaled by about hs / ha on its own).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "phaze_amd.h"

#define PI 3.14159265358979323846

static int fail(const char *what, int rc, const pv_stretch *h)
{
    fprintf(stderr, "%s: %s (%s)\n", what, pv_status_string(rc), pv_stretch_last_error(h));
    return 1;
}

/* the phase p of y[n] ~ a cos(w n) + b sin(w n) = A cos(w n + p) over [lo, hi): 2 x 2 least squares */
static double fit_phase(const float *y, long lo, long hi, double w)
{
    double cc = 0, cs = 0, ss = 0, yc = 0, ys = 0, det, a, b;
    long n;
    for (n = lo; n < hi; n++) {
        const double c = cos(w * (double)n), s = sin(w * (double)n);
        cc += c * c; cs += c * s; ss += s * s;
        yc += y[n] * c; ys += y[n] * s;
    }
    det = cc * ss - cs * cs;
    a = (yc * ss - ys * cs) / det;
    b = (ys * cc - yc * cs) / det;
    return atan2(-b, a);
}

static double offset_deg(const float *out, long nout, long lo, double w)
{
    double d = fit_phase(out + nout, lo, nout - 1024, w) - fit_phase(out, lo, nout - 1024, w);
    while (d > PI) d -= 2 * PI;
    while (d <= -PI) d += 2 * PI;
    return d * 180.0 / PI;
}

int main(int argc, char **argv)
{
    pv_stretch_config cfg = PV_STRETCH_CONFIG_INIT;
    const int N = argc > 1 ? atoi(argv[1]) : 1024;
    const int ha = argc > 2 ? atoi(argv[2]) : 205;
    const int hs = argc > 3 ? atoi(argv[3]) : 256;
    const int nframes = argc > 4 ? atoi(argv[4]) : 400;
    const double w = 2.0 * PI * 64.37 / 1024.0;            /* 64.37 bins of a 1024-point frame */
    pv_stretch *linked = NULL, *unlinked = NULL;
    float *in, *out;
    long i, nin, nout, lo;
    int rc;
    if (nframes <= 0 || ha < 1 || hs < 1) {
        fprintf(stderr, "need nframes, analysis_hop and synthesis_hop > 0\n");
        return 2;
    }
    nin = (long)nframes * ha;
    nout = (long)nframes * hs;
    lo = (long)((N + ha - 1) / ha + 2) * hs + N;           /* past the onset */
    if (nout - 1024 - lo < 4L * N) {
        fprintf(stderr, "too few frames for a steady output\n");
        return 2;
    }
    cfg.fft_size = N;
    cfg.analysis_hop = ha;
    cfg.synthesis_hop = hs;
    cfg.max_channels = 2;
    cfg.max_frames = nframes;
    rc = pv_stretch_create(&cfg, &linked);
    if (rc != PV_OK) return fail("pv_stretch_create", rc, NULL);
    rc = pv_link_channels(linked, 2);
    if (rc != PV_OK) return fail("pv_link_channels", rc, linked);
    rc = pv_stretch_create(&cfg, &unlinked);
    if (rc != PV_OK) return fail("pv_stretch_create", rc, NULL);
    in = (float *)malloc(sizeof(float) * 2 * (size_t)nin);
    out = (float *)malloc(sizeof(float) * 2 * (size_t)nout);
    if (!in || !out) {
        fprintf(stderr, "out of memory\n");
        return 1;
    }
    for (i = 0; i < nin; i++) {
        in[i] = (float)(0.5 * cos(w * (double)i));                  /* left */
        in[nin + i] = (float)(0.5 * cos(w * (double)i + PI / 2));  /* right: 90 degrees ahead */
    }
    rc = pv_stretch_process(linked, in, out, 2, nframes, nin, nout);
    if (rc != PV_OK) return fail("pv_stretch_process", rc, linked);
    printf("stretch: %d -> %d (%.4fx), fft_size %d\n", ha, hs, (double)hs / ha, N);
    printf("input offset deg: 90\n");
    printf("linked offset deg: %.6f\n", offset_deg(out, nout, lo, w));
    rc = pv_stretch_process(unlinked, in, out, 2, nframes, nin, nout);
    if (rc != PV_OK) return fail("pv_stretch_process", rc, unlinked);
    printf("unlinked offset deg: %.6f\n", offset_deg(out, nout, lo, w));
    pv_stretch_destroy(linked);
    pv_stretch_destroy(unlinked);
    free(in);
    free(out);
    return 0;
}
