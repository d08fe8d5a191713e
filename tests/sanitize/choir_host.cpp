// choir_host.cpp -- a stand-alone driver of the host code behind pv_choir_*: the planner (pv_choir_plan.hip) and the validation and tile walk of
// pv_choir.h, on the CPU, with no device.  tests/test_choir_abi.py builds it with -fsanitize=address,undefined, feeds it tables and tracks and
// compares what it prints with tests/choir_model.py exactly.  Every buffer is allocated at its exact size, so that a write past the capacity or a read
// past a table is an error the sanitizer reports.
//   choir_host tiles FILE NGRAINS MAX_PERIOD OUT_FIRST NOUT
//       FILE: int32[NGRAINS][4], ONE voice's table.  Prints "bad G WHY" for a table that is refused, else one line "A B SRC0 COUNT SRC0_AS_UPLOADED" per tile.
//   choir_host plan FILE NREC HOP CENTER INPUT_LEN UNVOICED MIN_PERIOD MAX_PERIOD WITH_WARPS WITH_EPOCHS MIN_STRENGTH LOCK MIRROR
//       FILE: int32[NREC][4] f0 records, double[NREC] ratios, double[NREC] rates, double[NREC] warps, int32[NREC][4] epoch records.  Sizes in two calls;
//       prints "n N OUTPUT_LEN" and one line "T W D L" per grain, or "refused RC".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/phaze_amd.h"
#include "../../phaze_amd/csrc/psola/pv_choir.h"

static bool read_exact(FILE *f, void *to, size_t bytes) { return bytes == 0 || fread(to, 1, bytes, f) == bytes; }

static int run_tiles(int argc, char **argv)
{
    if (argc != 7) return 2;
    const long long ng = atoll(argv[3]), mp = atoll(argv[4]), first = atoll(argv[5]), nout = atoll(argv[6]);
    FILE *f = fopen(argv[2], "rb");
    if (!f || ng < 0 || nout < 0) return 2;
    int32_t *g = (int32_t *)malloc(ng > 0 ? sizeof(int32_t) * 4 * (size_t)ng : 1);
    const bool ok = read_exact(f, g, sizeof(int32_t) * 4 * (size_t)ng);
    fclose(f);
    if (!ok) { free(g); return 2; }
    int why = 0;
    const int64_t bad = pv_choir_check_grains(g, ng, (int)mp, &why);
    if (bad >= 0) {
        printf("bad %lld %d\n", (long long)bad, why);
    } else {
        const long long ntiles = (nout + PV_TSM_TILE - 1) / PV_TSM_TILE;
        int64_t *t = (int64_t *)malloc(ntiles > 0 ? sizeof(int64_t) * 4 * (size_t)ntiles : 1);
        if (pv_choir_tiles(g, ng, (int)mp, first, nout, t) != ntiles) return 3;
        for (long long k = 0; k < ntiles; k++)
            printf("%lld %lld %lld %lld %d\n", (long long)t[4 * k], (long long)t[4 * k + 1], (long long)t[4 * k + 2], (long long)t[4 * k + 3], (int)pv_choir_src0(t[4 * k + 2]));
        free(t);
    }
    free(g);
    return 0;
}

static int run_plan(int argc, char **argv)
{
    if (argc != 15) return 2;
    const long long nrec = atoll(argv[3]);
    pv_psola_params p = PV_PSOLA_PARAMS_INIT;
    pv_epoch_params e = PV_EPOCH_PARAMS_INIT;
    p.f0_hop = atoi(argv[4]); p.f0_center = atoi(argv[5]); p.input_len = atoll(argv[6]); p.unvoiced_period = atof(argv[7]);
    p.min_period = atoi(argv[8]); p.max_period = atoi(argv[9]);
    const int with_warps = atoi(argv[10]), with_epochs = atoi(argv[11]);
    e.min_strength = atoi(argv[12]); e.lock = atof(argv[13]);
    const int mirror = atoi(argv[14]);
    FILE *f = fopen(argv[2], "rb");
    if (!f || nrec < 0) return 2;
    const size_t n = (size_t)nrec;
    int32_t *rec = (int32_t *)malloc(n ? sizeof(int32_t) * 4 * n : 1), *ep = (int32_t *)malloc(n ? sizeof(int32_t) * 4 * n : 1);
    double *ratios = (double *)malloc(n ? sizeof(double) * n : 1), *rates = (double *)malloc(n ? sizeof(double) * n : 1), *warps = (double *)malloc(n ? sizeof(double) * n : 1);
    const bool ok = read_exact(f, rec, sizeof(int32_t) * 4 * n) && read_exact(f, ratios, sizeof(double) * n) && read_exact(f, rates, sizeof(double) * n)
                    && read_exact(f, warps, sizeof(double) * n) && read_exact(f, ep, sizeof(int32_t) * 4 * n);
    fclose(f);
    int rc = 2;
    if (ok) {
        int64_t len = -1;
        const double *wp = with_warps ? warps : NULL;
        const int32_t *epp = with_epochs ? ep : NULL;
        const int64_t m = pv_choir_plan(&p, &e, n ? rec : NULL, nrec, ratios, rates, wp, epp, mirror, NULL, 0, &len);
        rc = 0;
        if (m < 0) {
            printf("refused %lld\n", (long long)m);
        } else {
            int32_t *g = (int32_t *)malloc(m > 0 ? sizeof(int32_t) * 4 * (size_t)m : 1);         // exactly the capacity
            int64_t len2 = -1;
            if (pv_choir_plan(&p, &e, n ? rec : NULL, nrec, ratios, rates, wp, epp, mirror, g, m, &len2) != m || len2 != len) rc = 3;
            // a smaller capacity writes no more than it
            if (m > 3) {
                int32_t *s = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)(m - 3));
                if (pv_choir_plan(&p, &e, n ? rec : NULL, nrec, ratios, rates, wp, epp, mirror, s, m - 3, NULL) != m || memcmp(s, g, sizeof(int32_t) * 4 * (size_t)(m - 3)) != 0)
                    rc = 3;
                free(s);
            }
            printf("n %lld %lld\n", (long long)m, (long long)len);
            for (int64_t k = 0; k < m; k++) printf("%d %d %d %d\n", g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
            free(g);
        }
    }
    free(rec); free(ep); free(ratios); free(rates); free(warps);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "tiles")) return run_tiles(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "plan")) return run_plan(argc, argv);
    fprintf(stderr, "usage: choir_host tiles ... | plan ... (see the head of tests/sanitize/choir_host.cpp)\n");
    return 2;
}
