/*
 * trace_smoke.c -- a plain C caller of the ray queries of include/bih.h
 * (test infrastructure): bih_build, then bih_trace for both queries.
 *
 *   trace_smoke --errors                     device-free error codes only
 *   trace_smoke SCENE.f32 N RAYS.bin NRAYS HITS.bin
 *       SCENE.f32  N*9 float32 (file order), RAYS.bin NRAYS bih_ray records;
 *       writes NRAYS bih_hit records (closest), then NRAYS bytes (occluded)
 *
 * Exit 0 = every check passed; prints one line per check.  Built by
 * tests/test_trace.py with gcc -std=c11 -Wall -Wextra -Werror -pedantic
 * against -lbih_amd.
 */
#include "bih.h"

#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(bih_ray) == 32, "bih_ray is 32 bytes");
_Static_assert(sizeof(bih_hit) == 16, "bih_hit is 16 bytes");

static int g_fail = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (cond) {                                        \
            printf("ok   ");                               \
        } else {                                           \
            printf("FAIL ");                               \
            g_fail = 1;                                    \
        }                                                  \
        printf(__VA_ARGS__);                               \
        printf("\n");                                      \
    } while (0)

static void *read_file(const char *path, size_t bytes) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    void *p = malloc(bytes ? bytes : 1);
    size_t got = p ? fread(p, 1, bytes, f) : 0;
    fclose(f);
    if (got != bytes) { free(p); return NULL; }
    return p;
}

/* The argument checks come before the tree is touched, so a stand-in tree
 * pointer (never dereferenced on these paths) reaches each of them. */
static void check_errors(void) {
    static bih_ray ray;
    static bih_hit hit;
    const bih_tree *fake = (const bih_tree *)(const void *)&ray;
    CHECK(bih_trace(NULL, &ray, 1, BIH_QUERY_CLOSEST, &hit) == BIH_ERR_INVALID, "bih_trace(NULL tree) -> INVALID");
    CHECK(bih_trace_device(NULL, &ray, 1, BIH_QUERY_CLOSEST, &hit, NULL) == BIH_ERR_INVALID,
          "bih_trace_device(NULL tree) -> INVALID");
    CHECK(bih_trace(fake, NULL, 1, BIH_QUERY_CLOSEST, &hit) == BIH_ERR_INVALID &&
              bih_trace_device(fake, NULL, 1, BIH_QUERY_CLOSEST, &hit, NULL) == BIH_ERR_INVALID,
          "NULL rays -> INVALID");
    CHECK(bih_trace(fake, &ray, 1, BIH_QUERY_OCCLUDED, NULL) == BIH_ERR_INVALID &&
              bih_trace_device(fake, &ray, 1, BIH_QUERY_OCCLUDED, NULL, NULL) == BIH_ERR_INVALID,
          "NULL out -> INVALID");
    CHECK(bih_trace(fake, &ray, 1, 2u, &hit) == BIH_ERR_INVALID &&
              bih_trace_device(fake, &ray, 1, 2u, &hit, NULL) == BIH_ERR_INVALID,
          "unknown query -> INVALID");
    CHECK(bih_trace(fake, &ray, (uint64_t)BIH_MAX_RAYS + 1u, BIH_QUERY_CLOSEST, &hit) == BIH_ERR_TOO_LARGE &&
              bih_trace_device(fake, &ray, (uint64_t)BIH_MAX_RAYS + 1u, BIH_QUERY_CLOSEST, &hit, NULL) ==
                  BIH_ERR_TOO_LARGE,
          "more than BIH_MAX_RAYS -> TOO_LARGE");
    CHECK(bih_trace(fake, NULL, 0, BIH_QUERY_CLOSEST, NULL) == BIH_OK &&
              bih_trace_device(fake, NULL, 0, BIH_QUERY_OCCLUDED, NULL, NULL) == BIH_OK,
          "no rays -> OK");
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--errors")) {
        check_errors();
        return g_fail;
    }
    if (argc != 6) {
        fprintf(stderr, "usage: trace_smoke SCENE.f32 N RAYS.bin NRAYS HITS.bin | --errors\n");
        return 2;
    }
    uint32_t n = (uint32_t)strtoul(argv[2], NULL, 10);
    size_t nrays = (size_t)strtoull(argv[4], NULL, 10);
    float *v = (float *)read_file(argv[1], (size_t)n * 9 * sizeof(float));
    bih_ray *rays = (bih_ray *)read_file(argv[3], nrays * sizeof(bih_ray));
    bih_hit *hits = (bih_hit *)calloc(nrays ? nrays : 1, sizeof(bih_hit));
    uint8_t *occ = (uint8_t *)calloc(nrays ? nrays : 1, 1);
    if (!v || !rays || !hits || !occ) { fprintf(stderr, "cannot read inputs\n"); return 2; }
    CHECK(bih_device_count() > 0, "device count %d", bih_device_count());
    if (g_fail) return 1;

    bih_scene scene = {n, v};
    bih_tree *tree = NULL;
    int rc = bih_build(&scene, 0, &tree);
    CHECK(rc == BIH_OK && tree, "bih_build: %s", bih_strerror(rc));
    if (rc) return 1;
    rc = bih_trace(tree, rays, nrays, BIH_QUERY_CLOSEST, hits);
    CHECK(rc == BIH_OK, "bih_trace closest, %zu rays: %s", nrays, bih_strerror(rc));
    rc = bih_trace(tree, rays, nrays, BIH_QUERY_OCCLUDED, occ);
    CHECK(rc == BIH_OK, "bih_trace occluded: %s", bih_strerror(rc));
    size_t nhit = 0, bad = 0;
    for (size_t i = 0; i < nrays; ++i) {
        const int hit = hits[i].prim != BIH_NO_HIT;
        nhit += (size_t)hit;
        bad += (size_t)(occ[i] != (uint8_t)hit);
        if (hit) bad += (size_t)(!(hits[i].t > rays[i].t_lo) || hits[i].prim >= n);
        else bad += (size_t)(hits[i].t != FLT_MAX || hits[i].u != 0.0f || hits[i].v != 0.0f);
    }
    CHECK(bad == 0, "%zu hits of %zu rays; %zu inconsistent records", nhit, nrays, bad);
    CHECK(bih_trace(tree, rays, 1, 7u, hits) == BIH_ERR_INVALID, "unknown query with a live tree -> INVALID");
    bih_free(tree);

    FILE *f = fopen(argv[5], "wb");
    int wrote = f && fwrite(hits, sizeof(bih_hit), nrays, f) == nrays && fwrite(occ, 1, nrays, f) == nrays;
    if (f) wrote = fclose(f) == 0 && wrote;
    CHECK(wrote, "results written to %s", argv[5]);
    free(occ); free(hits); free(rays); free(v);
    printf("%s\n", g_fail ? "trace_smoke FAILED" : "trace_smoke OK");
    return g_fail;
}
