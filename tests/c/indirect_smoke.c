/*
 * indirect_smoke.c -- a plain C caller of the one-bounce indirect-lighting
 * render of include/bih.h (test infrastructure): bih_build,
 * bih_camera_reference, bih_render_indirect, bih_bounce_sample.
 *
 *   indirect_smoke --errors                device-free error codes only
 *   indirect_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD LAMPS.f32 KP AREA.f32 KA ALBEDO SKY OUT.bin
 *       SCENE.f32  N*9 float32 (file order); DIR.f32  KD bih_light; LAMPS.f32
 *       KP bih_point_light; AREA.f32  KA bih_area_light; renders frame FRAME of
 *       the W x H image (reference camera, seed 1984) and writes, one after the
 *       other, lit (W*H*SPP u64), bounce (W*H*SPP bih_hit), lit2, irradiance, rgba
 *
 * Exit 0 = every check passed; prints one line per check.  Built by
 * tests/test_indirect.py with gcc -std=c11 -Wall -Wextra -Werror -pedantic
 * against -lbih_amd.
 */
#include "bih.h"

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(bih_bounce) == 8 && offsetof(bih_bounce, sky) == 4, "bih_bounce: albedo, sky");
_Static_assert(sizeof(bih_indirect) == 5 * sizeof(void *) && offsetof(bih_indirect, bounce) == sizeof(void *) &&
                   offsetof(bih_indirect, rgba) == 4 * sizeof(void *),
               "lit, bounce, lit2, irradiance, rgba");
_Static_assert(BIH_BOUNCE_SLOT == 0x80000000u && BIH_ABI_VERSION == 4, "constants");

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
                const bih_light_set *s, const bih_bounce *b, const bih_indirect *d, int expect) {
    return bih_render_indirect(t, c, w, h, spp, 0, 1984, rows, s, b, d) == expect &&
           bih_render_indirect_device(t, c, w, h, spp, 0, 1984, rows, s, b, d, NULL) == expect;
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
    const bih_bounce bn = {0.5f, 0.25f};
    const bih_indirect none = {NULL, NULL, NULL, NULL, NULL};
    bih_indirect rgba = none, hits = none, odd_lit2 = none, odd_hits = none;
    rgba.rgba = (uint32_t *)(void *)buf;
    hits.bounce = (bih_hit *)(void *)buf;
    odd_lit2.lit2 = (uint64_t *)(void *)((char *)buf + 4);
    odd_hits.bounce = (bih_hit *)(void *)((char *)buf + 8);
    const bih_rows outside = {6, 4, 4, 1}, empty = {0, 0, 1, 1};
    const bih_light_set full = set_of(sun, 1, lamp, 1, pan, 1), zero = set_of(NULL, 0, NULL, 0, NULL, 0);
    const bih_light_set many = set_of(sun, 33, lamp, 31, pan, 1), a17 = set_of(NULL, 0, NULL, 0, pan, 17);
    const bih_light_set na = set_of(sun, 1, lamp, 1, NULL, 1);
    CHECK(both(NULL, &cam, 8, 8, 4, NULL, &full, &bn, &rgba, BIH_ERR_INVALID) &&
              both(fake, NULL, 8, 8, 4, NULL, &full, &bn, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &full, &bn, NULL, BIH_ERR_INVALID),
          "NULL tree, camera or planes -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 65, NULL, &full, &bn, &rgba, BIH_ERR_INVALID), "spp > 64 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &full, &bn, &none, BIH_ERR_INVALID), "all five planes NULL -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &outside, &full, &bn, &rgba, BIH_ERR_INVALID), "bad rows -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &many, &bn, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &a17, &bn, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &na, &bn, &rgba, BIH_ERR_INVALID),
          "too many lights, too many panels, a NULL array with a count -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &full, NULL, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, &bn, &odd_lit2, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, &bn, &odd_hits, BIH_ERR_INVALID),
          "NULL bounce, misaligned lit2 or bounce plane -> INVALID (even with no rows)");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &full, &bn, &hits, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, &zero, &bn, &rgba, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, NULL, &bn, &rgba, BIH_OK),
          "nrows == 0 -> OK; an empty or NULL light set is legal (sky only)");
    /* the bounce direction: n + a unit vector, a function of every argument, and its checks */
    const float n[3] = {0.0f, 0.0f, 1.0f};
    float d[3] = {0.0f, 0.0f, 0.0f}, d2[3];
    const int bad = bih_bounce_sample(1984, 0, 0, 4, 0, NULL, d) == BIH_ERR_INVALID &&
                    bih_bounce_sample(1984, 0, 0, 4, 0, n, NULL) == BIH_ERR_INVALID &&
                    bih_bounce_sample(1984, 0, 0, 0, 0, n, d) == BIH_ERR_INVALID &&
                    bih_bounce_sample(1984, 0, 0, 4, 4, n, d) == BIH_ERR_INVALID;
    const int ok = bih_bounce_sample(1984, 5, 1, 4, 3, n, d) == BIH_OK && bih_bounce_sample(1984, 5, 1, 4, 2, n, d2) == BIH_OK;
    const float len2 = d[0] * d[0] + d[1] * d[1] + (d[2] - 1.0f) * (d[2] - 1.0f);
    CHECK(bad && ok && len2 > 0.9999f && len2 < 1.0001f && d[2] >= 0.0f && (d2[0] != d[0] || d2[2] != d[2]),
          "bih_bounce_sample: its checks; (%g, %g, %g) - n has length 1; sample 2 takes another", (double)d[0],
          (double)d[1], (double)d[2]);
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--errors")) {
        check_errors();
        return g_fail;
    }
    if (argc != 16) {
        fprintf(stderr, "usage: indirect_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD LAMPS.f32 KP AREA.f32 KA ALBEDO SKY"
                        " OUT.bin | --errors\n");
        return 2;
    }
    const uint32_t n = (uint32_t)strtoul(argv[2], NULL, 10);
    const uint32_t w = (uint32_t)strtoul(argv[3], NULL, 10), h = (uint32_t)strtoul(argv[4], NULL, 10);
    const uint32_t spp = (uint32_t)strtoul(argv[5], NULL, 10), frame = (uint32_t)strtoul(argv[6], NULL, 10);
    const uint32_t kd = (uint32_t)strtoul(argv[8], NULL, 10), kp = (uint32_t)strtoul(argv[10], NULL, 10);
    const uint32_t ka = (uint32_t)strtoul(argv[12], NULL, 10);
    const bih_bounce bn = {strtof(argv[13], NULL), strtof(argv[14], NULL)};
    const size_t P = (size_t)w * h, S = P * spp;
    float *v = (float *)read_file(argv[1], (size_t)n * 9 * sizeof(float));
    bih_light *dir = (bih_light *)read_file(argv[7], (size_t)kd * sizeof(bih_light));
    bih_point_light *lamps = (bih_point_light *)read_file(argv[9], (size_t)kp * sizeof(bih_point_light));
    bih_area_light *area = (bih_area_light *)read_file(argv[11], (size_t)ka * sizeof(bih_area_light));
    bih_indirect d;
    d.lit = (uint64_t *)calloc(S ? S : 1, sizeof(uint64_t));
    d.bounce = (bih_hit *)calloc(S ? S : 1, sizeof(bih_hit));
    d.lit2 = (uint64_t *)calloc(S ? S : 1, sizeof(uint64_t));
    d.irradiance = (float *)calloc(P ? P : 1, sizeof(float));
    d.rgba = (uint32_t *)calloc(P ? P : 1, sizeof(uint32_t));
    if (!v || !dir || !lamps || !area || !d.lit || !d.bounce || !d.lit2 || !d.irradiance || !d.rgba) {
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
    rc = bih_render_indirect(tree, &cam, w, h, spp, frame, 1984, NULL, &set, &bn, &d);
    CHECK(rc == BIH_OK, "bih_render_indirect %ux%ux%u frame %u, %u + %u + %u lights: %s", w, h, spp, frame, kd, kp, ka,
          bih_strerror(rc));
    /* a lit2 word belongs to a stopped bounce ray, a stopped bounce ray to a hit sample's pixel */
    size_t stopped = 0, bad = 0;
    for (size_t i = 0; i < S; ++i) {
        const int hit2 = d.bounce[i].prim != BIH_NO_HIT;
        stopped += (size_t)hit2;
        bad += (size_t)(d.lit2[i] != 0 && !hit2) + (size_t)(hit2 && d.bounce[i].prim >= n);
    }
    CHECK(bad == 0 && stopped > 0, "%zu stopped bounce rays of %zu samples; %zu inconsistent records", stopped, S, bad);
    bih_free(tree);

    FILE *f = fopen(argv[15], "wb");
    int wrote = f && fwrite(d.lit, 8, S, f) == S && fwrite(d.bounce, 16, S, f) == S && fwrite(d.lit2, 8, S, f) == S &&
                fwrite(d.irradiance, 4, P, f) == P && fwrite(d.rgba, 4, P, f) == P;
    if (f) wrote = fclose(f) == 0 && wrote;
    CHECK(wrote, "planes written to %s", argv[15]);
    free(d.rgba); free(d.irradiance); free(d.lit2); free(d.bounce); free(d.lit); free(area); free(lamps); free(dir);
    free(v);
    printf("%s\n", g_fail ? "indirect_smoke FAILED" : "indirect_smoke OK");
    return g_fail;
}
