/*
 * lights_smoke.c -- a plain C caller of the direct-lighting render with point
 * lights of include/bih.h (test infrastructure): bih_build,
 * bih_camera_reference, bih_render_lights; a segment-query ray too.
 *
 *   lights_smoke --errors                    device-free error codes only
 *   lights_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD LAMPS.f32 KP OUT.bin
 *       SCENE.f32  N*9 float32 (file order); DIR.f32  KD bih_light; LAMPS.f32
 *       KP bih_point_light; renders frame FRAME of the W x H image (reference
 *       camera, seed 1984) and writes, one after the other, lit (W*H*SPP u64),
 *       irradiance, rgba
 *
 * Exit 0 = every check passed; prints one line per check.  Built by
 * tests/test_lights.py with gcc -std=c11 -Wall -Wextra -Werror -pedantic
 * against -lbih_amd.
 */
#include "bih.h"

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(bih_point_light) == 16, "bih_point_light is 16 bytes");
_Static_assert(offsetof(bih_point_light, weight) == 12, "pos, then weight");
_Static_assert(sizeof(bih_ray) == 32, "bih_ray is 32 bytes");
_Static_assert(offsetof(bih_ray, t_hi) == 28 && offsetof(bih_ray, reserved) == 28, "one float, two names");
_Static_assert(BIH_QUERY_CLOSEST_WITHIN == 0x10u && BIH_QUERY_OCCLUDED_WITHIN == 0x11u, "segment query codes");

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
                const bih_light *l, uint32_t kd, const bih_point_light *q, uint32_t kp, const bih_direct *d,
                int expect) {
    return bih_render_lights(t, c, w, h, spp, 0, 1984, rows, l, kd, q, kp, d) == expect &&
           bih_render_lights_device(t, c, w, h, spp, 0, 1984, rows, l, kd, q, kp, d, NULL) == expect;
}

/* The argument checks come before the tree is touched, so a stand-in tree
 * pointer (never dereferenced on these paths) reaches each of them. */
static void check_errors(void) {
    static _Alignas(16) float buf[16];
    static bih_camera cam;
    static bih_light sun[1] = {{{0.0f, 1.0f, 0.0f}, 1.0f}};
    static bih_point_light lamp[1] = {{{0.0f, 1.0f, 0.0f}, 1.0f}};
    const bih_tree *fake = (const bih_tree *)(const void *)buf;
    bih_direct none = {NULL, NULL, NULL};
    bih_direct rgba = none, lit = none, odd = none;
    rgba.rgba = (uint32_t *)(void *)buf;
    lit.lit = (uint64_t *)(void *)buf;
    odd.rgba = (uint32_t *)(void *)buf;
    odd.lit = (uint64_t *)(void *)((char *)buf + 4);
    const bih_rows outside = {6, 4, 4, 1}, empty = {0, 0, 1, 1};
    CHECK(both(NULL, &cam, 8, 8, 4, NULL, sun, 1, lamp, 1, &rgba, BIH_ERR_INVALID), "NULL tree -> INVALID");
    CHECK(both(fake, NULL, 8, 8, 4, NULL, sun, 1, lamp, 1, &rgba, BIH_ERR_INVALID), "NULL camera -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, sun, 1, lamp, 1, NULL, BIH_ERR_INVALID), "NULL planes -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 65, NULL, sun, 1, lamp, 1, &rgba, BIH_ERR_INVALID), "spp > 64 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, sun, 1, lamp, 1, &none, BIH_ERR_INVALID), "all planes NULL -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &outside, sun, 1, lamp, 1, &rgba, BIH_ERR_INVALID), "bad rows -> INVALID");
    CHECK(both(fake, &cam, 1u << 16, 1u << 16, 1, NULL, NULL, 0, NULL, 0, &odd, BIH_ERR_TOO_LARGE),
          "TOO_LARGE comes before the lights and the alignment");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, NULL, 0, NULL, 0, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, sun, 0, lamp, 0, &rgba, BIH_ERR_INVALID),
          "no light at all -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, sun, 33, lamp, 32, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, sun, 0xFFFFFFFFu, lamp, 2, &rgba, BIH_ERR_INVALID),
          "more than BIH_MAX_LIGHTS together -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, NULL, 1, lamp, 1, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, sun, 1, NULL, 1, &rgba, BIH_ERR_INVALID),
          "a NULL array with a count -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, NULL, 0, NULL, 0, &rgba, BIH_ERR_INVALID),
          "the lights come before nrows == 0");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, sun, 1, lamp, 1, &odd, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, NULL, 0, lamp, 1, &odd, BIH_ERR_INVALID),
          "misaligned lit -> INVALID (even with no rows)");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, NULL, 0, lamp, 1, &lit, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, sun, 1, NULL, 0, &lit, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, sun, 32, lamp, 32, &rgba, BIH_OK),
          "nrows == 0 -> OK (an array may be NULL when its count is 0)");
    /* the segment queries pass bih_trace's checks; a neighbouring code does not */
    bih_ray ray = {{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 1.0f}, {0.0f}};
    ray.t_hi = 1.0f;
    CHECK(ray.reserved == 1.0f, "bih_ray.t_hi is bih_ray.reserved");
    CHECK(bih_trace(fake, &ray, 0, BIH_QUERY_OCCLUDED_WITHIN, buf) == BIH_OK &&
              bih_trace(fake, &ray, 0, BIH_QUERY_CLOSEST_WITHIN, buf) == BIH_OK &&
              bih_trace(fake, &ray, 0, 0x12u, buf) == BIH_ERR_INVALID,
          "segment query codes: 0x10, 0x11 accepted, 0x12 -> INVALID");
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--errors")) {
        check_errors();
        return g_fail;
    }
    if (argc != 12) {
        fprintf(stderr, "usage: lights_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD LAMPS.f32 KP OUT.bin | --errors\n");
        return 2;
    }
    const uint32_t n = (uint32_t)strtoul(argv[2], NULL, 10);
    const uint32_t w = (uint32_t)strtoul(argv[3], NULL, 10), h = (uint32_t)strtoul(argv[4], NULL, 10);
    const uint32_t spp = (uint32_t)strtoul(argv[5], NULL, 10), frame = (uint32_t)strtoul(argv[6], NULL, 10);
    const uint32_t kd = (uint32_t)strtoul(argv[8], NULL, 10), kp = (uint32_t)strtoul(argv[10], NULL, 10);
    const size_t P = (size_t)w * h, S = P * spp;
    float *v = (float *)read_file(argv[1], (size_t)n * 9 * sizeof(float));
    bih_light *dir = (bih_light *)read_file(argv[7], (size_t)kd * sizeof(bih_light));
    bih_point_light *lamps = (bih_point_light *)read_file(argv[9], (size_t)kp * sizeof(bih_point_light));
    bih_direct d;
    d.lit = (uint64_t *)calloc(S ? S : 1, sizeof(uint64_t));
    d.irradiance = (float *)calloc(P ? P : 1, sizeof(float));
    d.rgba = (uint32_t *)calloc(P ? P : 1, sizeof(uint32_t));
    if (!v || !dir || !lamps || !d.lit || !d.irradiance || !d.rgba) {
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
    rc = bih_render_lights(tree, &cam, w, h, spp, frame, 1984, NULL, kd ? dir : NULL, kd, kp ? lamps : NULL, kp, &d);
    CHECK(rc == BIH_OK, "bih_render_lights %ux%ux%u frame %u, %u + %u lights: %s", w, h, spp, frame, kd, kp,
          bih_strerror(rc));
    /* bits at kd + kp and above are 0 */
    const uint32_t k = kd + kp;
    const uint64_t high = k >= 64 ? 0 : ~(uint64_t)0 << k;
    size_t lit_samples = 0, bad = 0;
    for (size_t i = 0; i < S; ++i) {
        bad += (size_t)((d.lit[i] & high) != 0);
        lit_samples += (size_t)(d.lit[i] != 0);
    }
    CHECK(bad == 0, "%zu lit samples of %zu; %zu with a bit past the lights", lit_samples, S, bad);
    bih_free(tree);

    FILE *f = fopen(argv[11], "wb");
    int wrote = f && fwrite(d.lit, 8, S, f) == S && fwrite(d.irradiance, 4, P, f) == P && fwrite(d.rgba, 4, P, f) == P;
    if (f) wrote = fclose(f) == 0 && wrote;
    CHECK(wrote, "planes written to %s", argv[11]);
    free(d.rgba); free(d.irradiance); free(d.lit); free(lamps); free(dir); free(v);
    printf("%s\n", g_fail ? "lights_smoke FAILED" : "lights_smoke OK");
    return g_fail;
}
