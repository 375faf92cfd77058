/*
 * denoise_smoke.c -- a plain C caller of the denoiser of include/bih.h (test
 * infrastructure): bih_build, bih_camera_reference, bih_denoise.
 *
 *   denoise_smoke --errors                device-free error codes only
 *   denoise_smoke SCENE.f32 N W H RADIANCE.f32 DEPTH.f32 NORMAL.f32 PASSES SQUARINGS SIGMA_COLOUR SIGMA_PLANE
 *       SCENE.f32  N*9 float32 (file order); RADIANCE.f32  W*H*3, DEPTH.f32  W*H,
 *       NORMAL.f32  W*H*3 float32: a colour render's radiance and the G-buffer's
 *       planes of the W x H frame under the reference camera; filters the frame
 *       and prints "checksum %016llx": the sum, modulo 2^64, of (i + 1) * word_i
 *       over the 32-bit words of radiance_out and rgba_out, one after the other
 *
 * Exit 0 = every check passed; prints one line per check.  Built by
 * tests/test_denoise.py with gcc -std=c11 -Wall -Wextra -Werror -pedantic
 * against -lbih_amd.
 */
#include "bih.h"

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(bih_denoise_params) == 16 && offsetof(bih_denoise_params, passes) == 0 &&
                   offsetof(bih_denoise_params, normal_squarings) == 4 &&
                   offsetof(bih_denoise_params, sigma_colour) == 8 && offsetof(bih_denoise_params, sigma_plane) == 12,
               "passes, normal_squarings, sigma_colour, sigma_plane");
_Static_assert(BIH_DENOISE_MAX_PASSES == 8 && BIH_DENOISE_MAX_SQUARINGS == 8 && BIH_DENOISE_MAX_PIXELS == (1u << 28) &&
                   BIH_ABI_VERSION == 4,
               "constants");

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
static int both(const bih_tree *t, const bih_camera *c, uint32_t w, uint32_t h, const bih_denoise_params *p,
                const float *rad, const float *depth, const float *nrm, float *out, uint32_t *rgba, int expect) {
    return bih_denoise(t, c, w, h, p, rad, depth, nrm, out, rgba) == expect &&
           bih_denoise_device(t, c, w, h, p, rad, depth, nrm, out, rgba, NULL) == expect;
}

/* The argument checks come before the tree is touched, so a stand-in tree
 * pointer (never dereferenced on these paths) reaches each of them. */
static void check_errors(void) {
    static _Alignas(16) float buf[16];
    static bih_camera cam;
    const bih_tree *fake = (const bih_tree *)(const void *)buf;
    uint32_t *px = (uint32_t *)(void *)buf;
    const bih_denoise_params good = {3, 5, 2.0f, 0.05f}, none = {0, 5, 2.0f, 0.05f}, nine = {9, 5, 2.0f, 0.05f};
    const bih_denoise_params sq9 = {3, 9, 2.0f, 0.05f}, both_bad = {0, 9, 2.0f, 0.05f};
    CHECK(both(NULL, &cam, 8, 8, &good, buf, buf, buf, buf, px, BIH_ERR_INVALID) &&
              both(fake, NULL, 8, 8, &good, buf, buf, buf, buf, px, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, NULL, buf, buf, buf, buf, px, BIH_ERR_INVALID),
          "NULL tree, camera or params -> INVALID");
    CHECK(both(fake, &cam, 0, 8, &good, buf, buf, buf, buf, px, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 0, &good, buf, buf, buf, buf, px, BIH_ERR_INVALID),
          "w or h == 0 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, &none, buf, buf, buf, buf, px, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, &nine, buf, buf, buf, buf, px, BIH_ERR_INVALID),
          "passes 0 or 9 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, &sq9, buf, buf, buf, buf, px, BIH_ERR_INVALID), "normal_squarings 9 -> INVALID");
    CHECK(both(fake, &cam, 1u << 14, (1u << 14) + 1, &good, NULL, NULL, NULL, NULL, NULL, BIH_ERR_TOO_LARGE) &&
              both(fake, &cam, 1u << 16, 1u << 16, &good, buf, buf, buf, buf, px, BIH_ERR_TOO_LARGE),
          "w*h > 2^28 -> TOO_LARGE (before the planes are looked at; w*h = 2^32 does not wrap)");
    CHECK(both(fake, &cam, 1u << 16, 1u << 16, &both_bad, buf, buf, buf, buf, px, BIH_ERR_INVALID),
          "bad params with a frame that is too large -> INVALID (the params come first)");
    CHECK(both(fake, &cam, 8, 8, &good, NULL, buf, buf, buf, px, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, &good, buf, NULL, buf, buf, px, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, &good, buf, buf, NULL, buf, px, BIH_ERR_INVALID),
          "NULL radiance, depth or normal -> INVALID");
    CHECK(both(fake, &cam, 8, 8, &good, buf, buf, buf, NULL, NULL, BIH_ERR_INVALID), "both outputs NULL -> INVALID");
}

/* sum of (i + 1) * word_i, continued over the call's regions */
static uint64_t fold(uint64_t sum, uint64_t *i, const void *p, size_t bytes) {
    const uint32_t *w = (const uint32_t *)p;
    for (size_t k = 0; k < bytes / 4; ++k) sum += (++*i) * (uint64_t)w[k];
    return sum;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--errors")) {
        check_errors();
        return g_fail;
    }
    if (argc != 12) {
        fprintf(stderr, "usage: denoise_smoke SCENE.f32 N W H RADIANCE.f32 DEPTH.f32 NORMAL.f32 PASSES SQUARINGS"
                        " SIGMA_COLOUR SIGMA_PLANE | --errors\n");
        return 2;
    }
    const uint32_t n = (uint32_t)strtoul(argv[2], NULL, 10);
    const uint32_t w = (uint32_t)strtoul(argv[3], NULL, 10), h = (uint32_t)strtoul(argv[4], NULL, 10);
    bih_denoise_params prm;
    prm.passes = (uint32_t)strtoul(argv[8], NULL, 10);
    prm.normal_squarings = (uint32_t)strtoul(argv[9], NULL, 10);
    prm.sigma_colour = strtof(argv[10], NULL);
    prm.sigma_plane = strtof(argv[11], NULL);
    const size_t P = (size_t)w * h;
    float *v = (float *)read_file(argv[1], (size_t)n * 9 * sizeof(float));
    float *rad = (float *)read_file(argv[5], P * 3 * sizeof(float));
    float *depth = (float *)read_file(argv[6], P * sizeof(float));
    float *nrm = (float *)read_file(argv[7], P * 3 * sizeof(float));
    float *out = (float *)calloc(P ? 3 * P : 1, sizeof(float));
    float *inplace = (float *)malloc(P ? 3 * P * sizeof(float) : 1);
    uint32_t *rgba = (uint32_t *)calloc(P ? P : 1, sizeof(uint32_t));
    if (!v || !rad || !depth || !nrm || !out || !inplace || !rgba) {
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
    rc = bih_denoise(tree, &cam, w, h, &prm, rad, depth, nrm, out, rgba);
    CHECK(rc == BIH_OK, "bih_denoise %ux%u, %u passes, %u squarings, sigmas %g %g: %s", w, h, prm.passes,
          prm.normal_squarings, (double)prm.sigma_colour, (double)prm.sigma_plane, bih_strerror(rc));
    size_t differ = 0;
    for (size_t p = 0; p < 3 * P; ++p) differ += (size_t)(memcmp(rad + p, out + p, 4) != 0);
    CHECK(differ > 0, "%zu of %zu radiance values changed", differ, 3 * P);
    /* in place, radiance alone: the same bytes */
    memcpy(inplace, rad, 3 * P * sizeof(float));
    rc = bih_denoise(tree, &cam, w, h, &prm, inplace, depth, nrm, inplace, NULL);
    CHECK(rc == BIH_OK && memcmp(inplace, out, 3 * P * sizeof(float)) == 0, "in place, radiance_out alone: %s",
          bih_strerror(rc));
    bih_free(tree);

    uint64_t sum = 0, i = 0;
    sum = fold(sum, &i, out, P * 12);
    sum = fold(sum, &i, rgba, P * 4);
    printf("checksum %016llx\n", (unsigned long long)sum);
    free(rgba); free(inplace); free(out); free(nrm); free(depth); free(rad); free(v);
    printf("%s\n", g_fail ? "denoise_smoke FAILED" : "denoise_smoke OK");
    return g_fail;
}
