// contour_host.cpp -- a stand-alone driver of the host code behind the pitch contour tracker: the path search (pv_contour_path.hip), on the CPU, with no
// device.  tests/test_contour_abi.py builds it with -fsanitize=address,undefined, feeds it tables and compares what it prints with tests/contour_model.py
// exactly.  Every buffer is allocated at its exact size, so that a write past the records or a read past the table is an error the sanitizer reports.
//   contour_host FILE NREC K MAX_LAG BIAS UNVOICED_COST VOICING_COST JUMP_COST
//       FILE: int32[NREC][K][4].  Prints "refused RC", or one line "TAU CM C0 CP STATE" per frame; the records of a second call without the states must
//       be the same.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/phaze_amd.h"

int main(int argc, char **argv)
{
    if (argc != 9) {
        fprintf(stderr, "usage: contour_host FILE NREC K MAX_LAG BIAS UNVOICED_COST VOICING_COST JUMP_COST\n");
        return 2;
    }
    const long long nrec = atoll(argv[2]);
    pv_contour_params p = PV_CONTOUR_PARAMS_INIT;
    p.candidates = atoi(argv[3]); p.max_lag = atoi(argv[4]); p.bias = atoi(argv[5]);
    p.unvoiced_cost = atoi(argv[6]); p.voicing_cost = atoi(argv[7]); p.jump_cost = atoi(argv[8]);
    if (nrec < 0 || p.candidates < 1 || p.candidates > 8) return 2;
    const size_t n = (size_t)nrec, K = (size_t)p.candidates;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t *cand = (int32_t *)malloc(n ? sizeof(int32_t) * 4 * K * n : 1);
    const bool ok = n == 0 || fread(cand, 1, sizeof(int32_t) * 4 * K * n, f) == sizeof(int32_t) * 4 * K * n;
    fclose(f);
    if (!ok) { free(cand); return 2; }
    int32_t *rec = (int32_t *)malloc(n ? sizeof(int32_t) * 4 * n : 1), *rec2 = (int32_t *)malloc(n ? sizeof(int32_t) * 4 * n : 1);
    int32_t *st = (int32_t *)malloc(n ? sizeof(int32_t) * n : 1);
    int rc = pv_contour_path(&p, n ? cand : NULL, nrec, n ? rec : NULL, n ? st : NULL);
    int status = 0;
    if (rc != PV_OK) {
        printf("refused %d\n", rc);
    } else {
        if (pv_contour_path(&p, n ? cand : NULL, nrec, n ? rec2 : NULL, NULL) != PV_OK || (n && memcmp(rec, rec2, sizeof(int32_t) * 4 * n) != 0)) status = 3;
        for (size_t m = 0; m < n; m++) printf("%d %d %d %d %d\n", rec[4 * m], rec[4 * m + 1], rec[4 * m + 2], rec[4 * m + 3], st[m]);
    }
    free(cand); free(rec); free(rec2); free(st);
    return status;
}
