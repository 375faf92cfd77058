/*
 * area_smoke.c -- a plain C caller of the direct-lighting render with area
 * lights of include/bih.h (test infrastructure): bih_build,
 * bih_camera_reference, bih_render_area_lights, bih_area_light_sample.
 *
 *   area_smoke --errors                    device-free error codes only
 *   area_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD LAMPS.f32 KP AREA.f32 KA OUT.bin
 *       SCENE.f32  N*9 float32 (file order); DIR.f32  KD bih_light; LAMPS.f32
 *       KP bih_point_light; AREA.f32  KA bih_area_light; renders frame FRAME of
 *       the W x H image (reference camera, seed 1984) and writes, one after the
 *       other, lit (W*H*SPP u64), irradiance, rgba
 *
 * Exit 0 = every check passed; prints one line per check.  Built by
 * tests/test_area_lights.py with gcc -std=c11 -Wall -Wextra -Werror -pedantic
 * against -lbih_amd.
 */
#include "bih.h"

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(bih_area_light) == 48, "bih_area_light is 48 bytes");
_Static_assert(offsetof(bih_area_light, weight) == 12 && offsetof(bih_area_light, edge_u) == 16 &&
                   offsetof(bih_area_light, edge_v) == 32,
               "corner, weight, edge_u, reserved0, edge_v, reserved1");
_Static_assert(BIH_MAX_AREA_LIGHTS == 16 && BIH_MAX_LIGHTS == 64 && BIH_ABI_VERSION == 4, "limits");

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

static bih_light_set set_of(const bih_light *l, uint32_t kd, const bih_point_light *q, uint32_t kp,
                            const bih_area_light *a, uint32_t ka) {
    bih_light_set s;
    s.dir = l; s.n_dir = kd;
    s.point = q; s.n_point = kp;
    s.area = a; s.n_area = ka;
    return s;
}

/* Both entries with the same arguments. */
static int both(const bih_tree *t, const bih_camera *c, uint32_t w, uint32_t h, uint32_t spp, const bih_rows *rows,
                const bih_light_set *s, const bih_direct *d, int expect) {
    return bih_render_area_lights(t, c, w, h, spp, 0, 1984, rows, s, d) == expect &&
           bih_render_area_lights_device(t, c, w, h, spp, 0, 1984, rows, s, d, NULL) == expect;
}

/* The argument checks come before the tree is touched, so a stand-in tree
 * pointer (never dereferenced on these paths) reaches each of them. */
static void check_errors(void) {
    static _Alignas(16) float buf[16];
    static bih_camera cam;
    static bih_light sun[1] = {{{0.0f, 1.0f, 0.0f}, 1.0f}};
    static bih_point_light lamp[1] = {{{0.0f, 1.0f, 0.0f}, 1.0f}};
    static bih_area_light pan[1] = {{{0.0f, 1.0f, 0.0f}, 1.0f, {1.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 1.0f}, 0.0f}};
    const bih_tree *fake = (const bih_tree *)(const void *)buf;
    bih_direct none = {NULL, NULL, NULL};
    bih_direct rgba = none, lit = none, odd = none;
    rgba.rgba = (uint32_t *)(void *)buf;
    lit.lit = (uint64_t *)(void *)buf;
    odd.rgba = (uint32_t *)(void *)buf;
    odd.lit = (uint64_t *)(void *)((char *)buf + 4);
    const bih_rows outside = {6, 4, 4, 1}, empty = {0, 0, 1, 1};
    const bih_light_set full = set_of(sun, 1, lamp, 1, pan, 1), zero = set_of(NULL, 0, NULL, 0, NULL, 0);
    const bih_light_set many = set_of(sun, 33, lamp, 31, pan, 1), huge = set_of(sun, 0xFFFFFFFFu, lamp, 1, pan, 1);
    const bih_light_set a17 = set_of(NULL, 0, NULL, 0, pan, 17), b17 = set_of(sun, 1, lamp, 1, pan, 17);
    const bih_light_set nd = set_of(NULL, 1, lamp, 1, pan, 1), np = set_of(sun, 1, NULL, 1, pan, 1);
    const bih_light_set na = set_of(sun, 1, lamp, 1, NULL, 1), only = set_of(NULL, 0, NULL, 0, pan, 1);
    const bih_light_set top = set_of(sun, 46, lamp, 2, pan, 16), dir = set_of(sun, 1, NULL, 0, NULL, 0);
    CHECK(both(NULL, &cam, 8, 8, 4, NULL, &full, &rgba, BIH_ERR_INVALID), "NULL tree -> INVALID");
    CHECK(both(fake, NULL, 8, 8, 4, NULL, &full, &rgba, BIH_ERR_INVALID), "NULL camera -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &full, NULL, BIH_ERR_INVALID), "NULL planes -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 65, NULL, &full, &rgba, BIH_ERR_INVALID), "spp > 64 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &full, &none, BIH_ERR_INVALID), "all planes NULL -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &outside, &full, &rgba, BIH_ERR_INVALID), "bad rows -> INVALID");
    CHECK(both(fake, &cam, 1u << 16, 1u << 16, 1, NULL, NULL, &odd, BIH_ERR_TOO_LARGE),
          "TOO_LARGE comes before the lights and the alignment");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, NULL, &rgba, BIH_ERR_INVALID), "NULL light set -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &zero, &rgba, BIH_ERR_INVALID), "no light at all -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &many, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &huge, &rgba, BIH_ERR_INVALID),
          "more than BIH_MAX_LIGHTS together -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &a17, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &b17, &rgba, BIH_ERR_INVALID),
          "more than BIH_MAX_AREA_LIGHTS panels -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &nd, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &np, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &na, &rgba, BIH_ERR_INVALID),
          "a NULL array with a count -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &zero, &rgba, BIH_ERR_INVALID), "the lights come before nrows == 0");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &full, &odd, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &only, &odd, BIH_ERR_INVALID),
          "misaligned lit -> INVALID (even with no rows)");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &only, &lit, BIH_OK) && both(fake, &cam, 8, 8, 4, &empty, &dir, &lit, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, &top, &rgba, BIH_OK),
          "nrows == 0 -> OK (an array may be NULL when its count is 0)");
    /* the sample point: on the panel, a function of every argument, and its checks */
    float q[3] = {0.0f, 0.0f, 0.0f}, q2[3];
    CHECK(bih_area_light_sample(NULL, 0, 1984, 0, 0, 4, 0, q) == BIH_ERR_INVALID &&
              bih_area_light_sample(pan, 0, 1984, 0, 0, 4, 0, NULL) == BIH_ERR_INVALID &&
              bih_area_light_sample(pan, 0, 1984, 0, 0, 0, 0, q) == BIH_ERR_INVALID &&
              bih_area_light_sample(pan, 0, 1984, 0, 0, 4, 4, q) == BIH_ERR_INVALID,
          "bih_area_light_sample: NULL light or q, spp == 0, s >= spp -> INVALID");
    CHECK(bih_area_light_sample(pan, 0, 1984, 5, 1, 4, 3, q) == BIH_OK && q[0] >= 0.0f && q[0] < 1.0f && q[1] == 1.0f &&
              q[2] >= 0.0f && q[2] < 1.0f && bih_area_light_sample(pan, 1, 1984, 5, 1, 4, 3, q2) == BIH_OK &&
              (q2[0] != q[0] || q2[2] != q[2]),
          "bih_area_light_sample: (%g, %g, %g) lies on the panel; light 1 takes another point", (double)q[0],
          (double)q[1], (double)q[2]);
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--errors")) {
        check_errors();
        return g_fail;
    }
    if (argc != 14) {
        fprintf(stderr, "usage: area_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD LAMPS.f32 KP AREA.f32 KA OUT.bin"
                        " | --errors\n");
        return 2;
    }
    const uint32_t n = (uint32_t)strtoul(argv[2], NULL, 10);
    const uint32_t w = (uint32_t)strtoul(argv[3], NULL, 10), h = (uint32_t)strtoul(argv[4], NULL, 10);
    const uint32_t spp = (uint32_t)strtoul(argv[5], NULL, 10), frame = (uint32_t)strtoul(argv[6], NULL, 10);
    const uint32_t kd = (uint32_t)strtoul(argv[8], NULL, 10), kp = (uint32_t)strtoul(argv[10], NULL, 10);
    const uint32_t ka = (uint32_t)strtoul(argv[12], NULL, 10);
    const size_t P = (size_t)w * h, S = P * spp;
    float *v = (float *)read_file(argv[1], (size_t)n * 9 * sizeof(float));
    bih_light *dir = (bih_light *)read_file(argv[7], (size_t)kd * sizeof(bih_light));
    bih_point_light *lamps = (bih_point_light *)read_file(argv[9], (size_t)kp * sizeof(bih_point_light));
    bih_area_light *area = (bih_area_light *)read_file(argv[11], (size_t)ka * sizeof(bih_area_light));
    bih_direct d;
    d.lit = (uint64_t *)calloc(S ? S : 1, sizeof(uint64_t));
    d.irradiance = (float *)calloc(P ? P : 1, sizeof(float));
    d.rgba = (uint32_t *)calloc(P ? P : 1, sizeof(uint32_t));
    if (!v || !dir || !lamps || !area || !d.lit || !d.irradiance || !d.rgba) {
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
    const bih_light_set set = set_of(kd ? dir : NULL, kd, kp ? lamps : NULL, kp, ka ? area : NULL, ka);
    rc = bih_render_area_lights(tree, &cam, w, h, spp, frame, 1984, NULL, &set, &d);
    CHECK(rc == BIH_OK, "bih_render_area_lights %ux%ux%u frame %u, %u + %u + %u lights: %s", w, h, spp, frame, kd, kp,
          ka, bih_strerror(rc));
    /* bits at kd + kp + ka and above are 0 */
    const uint32_t k = kd + kp + ka;
    const uint64_t high = k >= 64 ? 0 : ~(uint64_t)0 << k;
    size_t lit_samples = 0, bad = 0;
    for (size_t i = 0; i < S; ++i) {
        bad += (size_t)((d.lit[i] & high) != 0);
        lit_samples += (size_t)(d.lit[i] != 0);
    }
    CHECK(bad == 0, "%zu lit samples of %zu; %zu with a bit past the lights", lit_samples, S, bad);
    bih_free(tree);

    FILE *f = fopen(argv[13], "wb");
    int wrote = f && fwrite(d.lit, 8, S, f) == S && fwrite(d.irradiance, 4, P, f) == P && fwrite(d.rgba, 4, P, f) == P;
    if (f) wrote = fclose(f) == 0 && wrote;
    CHECK(wrote, "planes written to %s", argv[13]);
    free(d.rgba); free(d.irradiance); free(d.lit); free(area); free(lamps); free(dir); free(v);
    printf("%s\n", g_fail ? "area_smoke FAILED" : "area_smoke OK");
    return g_fail;
}
