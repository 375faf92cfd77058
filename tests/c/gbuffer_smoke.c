/*
 * gbuffer_smoke.c -- a plain C caller of the G-buffer render of include/bih.h
 * (test infrastructure): bih_build, bih_camera_reference, bih_render_gbuffer.
 *
 *   gbuffer_smoke --errors                   device-free error codes only
 *   gbuffer_smoke SCENE.f32 N W H SPP FRAME OUT.bin
 *       SCENE.f32  N*9 float32 (file order); renders frame FRAME of the W x H
 *       image (reference camera, seed 1984) and writes, one after the other,
 *       hits (W*H*SPP bih_hit), depth, prim, bary, normal, coverage
 *
 * Exit 0 = every check passed; prints one line per check.  Built by
 * tests/test_gbuffer.py with gcc -std=c11 -Wall -Wextra -Werror -pedantic
 * against -lbih_amd.
 */
#include "bih.h"

#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(bih_gbuffer) == 6 * sizeof(void *), "bih_gbuffer is six pointers");

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

/* Both entries with the same arguments. */
static int both(const bih_tree *t, const bih_camera *c, uint32_t w, uint32_t h, uint32_t spp, const bih_rows *rows,
                const bih_gbuffer *g, int expect) {
    return bih_render_gbuffer(t, c, w, h, spp, 0, 1984, rows, g) == expect &&
           bih_render_gbuffer_device(t, c, w, h, spp, 0, 1984, rows, g, NULL) == expect;
}

/* The argument checks come before the tree is touched, so a stand-in tree
 * pointer (never dereferenced on these paths) reaches each of them. */
static void check_errors(void) {
    static _Alignas(16) float buf[16];
    static bih_camera cam;
    const bih_tree *fake = (const bih_tree *)(const void *)buf;
    bih_gbuffer none = {NULL, NULL, NULL, NULL, NULL, NULL};
    bih_gbuffer depth = none, hits = none, odd = none;
    depth.depth = buf;
    hits.hits = (bih_hit *)(void *)buf;
    odd.depth = buf;
    odd.hits = (bih_hit *)(void *)((char *)buf + 4);
    const bih_rows zero_band = {0, 4, 0, 1}, outside = {6, 4, 4, 1}, empty = {0, 0, 1, 1};
    CHECK(both(NULL, &cam, 8, 8, 4, NULL, &depth, BIH_ERR_INVALID), "NULL tree -> INVALID");
    CHECK(both(fake, NULL, 8, 8, 4, NULL, &depth, BIH_ERR_INVALID), "NULL camera -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, NULL, BIH_ERR_INVALID), "NULL planes -> INVALID");
    CHECK(both(fake, &cam, 0, 8, 4, NULL, &depth, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 0, 4, NULL, &depth, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 0, NULL, &depth, BIH_ERR_INVALID),
          "w, h or spp == 0 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 65, NULL, &depth, BIH_ERR_INVALID), "spp > 64 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &none, BIH_ERR_INVALID), "all planes NULL -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &zero_band, &depth, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &outside, &depth, BIH_ERR_INVALID),
          "bad rows -> INVALID");
    CHECK(both(fake, &cam, 1u << 16, 1u << 16, 1, NULL, &depth, BIH_ERR_TOO_LARGE), "h*w*spp too large -> TOO_LARGE");
    CHECK(both(fake, &cam, 1u << 16, 1u << 16, 1, NULL, &odd, BIH_ERR_TOO_LARGE), "TOO_LARGE comes before the alignment");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &odd, BIH_ERR_INVALID) && both(fake, &cam, 8, 8, 4, &empty, &odd, BIH_ERR_INVALID),
          "misaligned hits -> INVALID (even with no rows)");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &hits, BIH_OK), "nrows == 0 -> OK");
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--errors")) {
        check_errors();
        return g_fail;
    }
    if (argc != 8) {
        fprintf(stderr, "usage: gbuffer_smoke SCENE.f32 N W H SPP FRAME OUT.bin | --errors\n");
        return 2;
    }
    const uint32_t n = (uint32_t)strtoul(argv[2], NULL, 10);
    const uint32_t w = (uint32_t)strtoul(argv[3], NULL, 10), h = (uint32_t)strtoul(argv[4], NULL, 10);
    const uint32_t spp = (uint32_t)strtoul(argv[5], NULL, 10), frame = (uint32_t)strtoul(argv[6], NULL, 10);
    const size_t P = (size_t)w * h;
    float *v = (float *)read_file(argv[1], (size_t)n * 9 * sizeof(float));
    bih_gbuffer g;
    const size_t S = P * spp;
    g.hits = (bih_hit *)calloc(S ? S : 1, sizeof(bih_hit));
    g.depth = (float *)calloc(P ? P : 1, sizeof(float));
    g.prim = (uint32_t *)calloc(P ? P : 1, sizeof(uint32_t));
    g.bary = (float *)calloc(P ? 2 * P : 1, sizeof(float));
    g.normal = (float *)calloc(P ? 3 * P : 1, sizeof(float));
    g.coverage = (uint32_t *)calloc(P ? P : 1, sizeof(uint32_t));
    if (!v || !g.hits || !g.depth || !g.prim || !g.bary || !g.normal || !g.coverage) {
        fprintf(stderr, "cannot read inputs\n");
        return 2;
    }
    CHECK(bih_device_count() > 0, "device count %d", bih_device_count());
    if (g_fail) return 1;

    bih_scene scene = {n, v};
    bih_tree *tree = NULL;
    bih_camera cam;
    int rc = bih_build(&scene, 0, &tree);
    CHECK(rc == BIH_OK && tree, "bih_build: %s", bih_strerror(rc));
    if (rc) return 1;
    rc = bih_camera_reference(w, h, &cam);
    CHECK(rc == BIH_OK, "bih_camera_reference: %s", bih_strerror(rc));
    rc = bih_render_gbuffer(tree, &cam, w, h, spp, frame, 1984, NULL, &g);
    CHECK(rc == BIH_OK, "bih_render_gbuffer %ux%ux%u frame %u: %s", w, h, spp, frame, bih_strerror(rc));
    size_t covered = 0, bad = 0;
    for (size_t p = 0; p < P; ++p) {
        uint32_t cnt = 0;
        float tmin = FLT_MAX;
        for (uint32_t s = 0; s < spp; ++s) {
            const bih_hit *q = &g.hits[p * spp + s];
            if (q->prim != BIH_NO_HIT) {
                ++cnt;
                if (q->t < tmin) tmin = q->t;
                bad += (size_t)(!(q->t > 0.0f) || q->prim >= n);
            } else {
                bad += (size_t)(q->t != FLT_MAX || q->u != 0.0f || q->v != 0.0f);
            }
        }
        covered += (size_t)(cnt > 0);
        bad += (size_t)(g.coverage[p] != cnt || g.depth[p] != tmin || (cnt == 0) != (g.prim[p] == BIH_NO_HIT));
        if (cnt == 0) bad += (size_t)(g.normal[3 * p] != 0.0f || g.normal[3 * p + 1] != 0.0f || g.normal[3 * p + 2] != 0.0f);
    }
    CHECK(bad == 0, "%zu covered pixels of %zu; %zu inconsistent records", covered, P, bad);
    bih_gbuffer none = {NULL, NULL, NULL, NULL, NULL, NULL};
    CHECK(bih_render_gbuffer(tree, &cam, w, h, spp, frame, 1984, NULL, &none) == BIH_ERR_INVALID,
          "all planes NULL with a live tree -> INVALID");
    bih_free(tree);

    FILE *f = fopen(argv[7], "wb");
    int wrote = f && fwrite(g.hits, sizeof(bih_hit), S, f) == S && fwrite(g.depth, 4, P, f) == P &&
                fwrite(g.prim, 4, P, f) == P && fwrite(g.bary, 4, 2 * P, f) == 2 * P &&
                fwrite(g.normal, 4, 3 * P, f) == 3 * P && fwrite(g.coverage, 4, P, f) == P;
    if (f) wrote = fclose(f) == 0 && wrote;
    CHECK(wrote, "planes written to %s", argv[7]);
    free(g.coverage); free(g.normal); free(g.bary); free(g.prim); free(g.depth); free(g.hits); free(v);
    printf("%s\n", g_fail ? "gbuffer_smoke FAILED" : "gbuffer_smoke OK");
    return g_fail;
}
