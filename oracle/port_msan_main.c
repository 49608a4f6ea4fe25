/* TEST INFRASTRUCTURE ONLY.  Stand-alone MemorySanitizer walk of the restatement over the small-set families (`make -C oracle msan`).
 *
 * The unmodified reference reads uninitialised memory in the 4-point branch of u2h (Htools.c:106-114); dg_oracle.c zero-fills there.
 * This program proves the restatement reads nothing it did not write on the inputs of tests/small_sets.py: it is compiled together
 * with dg_oracle.c under -fsanitize=memory, linked against libc and libm only, and calls the three drivers on every case of a dump
 * written by tests.small_sets.dump().  Outputs live in fresh (poisoned) heap blocks and are checked for being fully written.  Never
 * loaded into Python, never run on a GPU machine, not a pytest test.
 *
 * Dump: a version-1 .npy file of float64, one record per case:
 *   kind (0 H, 1 F, 2 ransacH2el), n, dim, seed, p[0..7], data
 *   H: p = px_th conf max_iters error_type sym_check laf_coef;        data = x1 [n, dim], x2 [n, dim]
 *   F: p = px_th conf max_iters error_type sym_check laf_coef degen;  data = x1 [n, dim], x2 [n, dim]
 *   E: p = th conf max_iters do_lo inl_limit;                          data = u10 [n, 10] */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dg_oracle.h"
#if defined(__has_feature)
#if __has_feature(memory_sanitizer)
#include <sanitizer/msan_interface.h>
#define CHECK_WRITTEN(p, bytes) __msan_check_mem_is_initialized((p), (bytes))
#define HAVE_MSAN 1
#endif
#endif
#ifndef HAVE_MSAN
#define CHECK_WRITTEN(p, bytes) ((void)0)
#define HAVE_MSAN 0
#endif

static double *read_npy(const char *path, size_t *count)
{
    FILE *f = fopen(path, "rb"); unsigned char head[10]; char *hdr; size_t hlen, bytes; long pos, end; double *d;
    if (!f) { perror(path); exit(2); }
    if (fread(head, 1, 10, f) != 10 || memcmp(head, "\x93NUMPY", 6) || head[6] != 1) { fprintf(stderr, "%s: not a version-1 .npy\n", path); exit(2); }
    hlen = head[8] | ((size_t)head[9] << 8);
    hdr = (char *)calloc(hlen + 1, 1);
    if (fread(hdr, 1, hlen, f) != hlen || !strstr(hdr, "'<f8'") || !strstr(hdr, "False")) { fprintf(stderr, "%s: want C-order float64\n", path); exit(2); }
    free(hdr);
    pos = ftell(f); fseek(f, 0, SEEK_END); end = ftell(f); fseek(f, pos, SEEK_SET);
    bytes = (size_t)(end - pos); d = (double *)malloc(bytes);
    if (fread(d, 1, bytes, f) != bytes) { fprintf(stderr, "%s: short read\n", path); exit(2); }
    fclose(f); *count = bytes / sizeof(double);
    return d;
}

int main(int argc, char **argv)
{
    size_t count, at = 0; double *d; long cases[3] = {0, 0, 0}, fit4[3] = {0, 0, 0}, fitshort[3] = {0, 0, 0}, found[3] = {0, 0, 0};
    if (argc != 2) { fprintf(stderr, "usage: %s small_sets.npy\n", argv[0]); return 2; }
    d = read_npy(argv[1], &count);
    while (at < count) {
        const double *r = d + at, *p = r + 4; int kind = (int)r[0], n = (int)r[1], dim = (int)r[2], k; unsigned seed = (unsigned)r[3];
        size_t len = 12 + (size_t)n * (size_t)(kind == 2 ? 10 : 2 * dim);
        /* fresh blocks, so that MemorySanitizer sees them as never written */
        double *M = (double *)malloc(9 * sizeof(double)); unsigned char *mask = (unsigned char *)malloc((size_t)n);
        int *st = (int *)malloc(DG_ST_COUNT * sizeof(int)); double acc = 0;
        if (kind < 0 || kind > 2 || n < 2 || at + len > count) { fprintf(stderr, "bad record at %zu\n", at); return 2; }
        if (kind == 0)
            dg_oracle_find_homography(r + 12, r + 12 + (size_t)n * dim, n, dim, p[0], p[1], (int)p[2], (int)p[3], (int)p[4], p[5], seed, M, mask, st);
        else if (kind == 1)
            dg_oracle_find_fundamental(r + 12, r + 12 + (size_t)n * dim, n, dim, p[0], p[1], (int)p[2], (int)p[3], (int)p[4], p[5], (int)p[6], seed, 0, M, mask, st);
        else
            dg_oracle_ransacH2el(r + 12, n, p[0], p[1], (int)p[2], (int)p[3], (int)p[4], seed, M, mask, st);
        CHECK_WRITTEN(M, 9 * sizeof(double)); CHECK_WRITTEN(mask, (size_t)n); CHECK_WRITTEN(st, (DG_ST_U2H_SHORT + 1) * sizeof(int));
        for (k = 0; k < 9; k++) acc += M[k] < 0 ? -M[k] : M[k];        /* a branch on every output number: reported if never written */
        cases[kind]++; found[kind] += acc > 0; fit4[kind] += st[DG_ST_U2H_4PT] > 0; fitshort[kind] += st[DG_ST_U2H_SHORT] > 0;
        free(M); free(mask); free(st); at += len;
    }
    for (at = 0; at < 3; at++)
        printf("%s: %ld cases, %ld with a model, %ld through the 4-point fit, %ld through the short-list fit\n",
               at == 0 ? "find_homography" : at == 1 ? "find_fundamental" : "ransacH2el", cases[at], found[at], fit4[at], fitshort[at]);
    printf("MemorySanitizer %s: no report\n", HAVE_MSAN ? "on" : "OFF (plain build)");
    free(d);
    return 0;
}
