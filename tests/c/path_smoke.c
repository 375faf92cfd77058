/*
 * path_smoke.c -- a plain C caller of the multi-bounce path render of
 * include/bih.h (test infrastructure): bih_build, bih_camera_reference,
 * bih_render_path, bih_path_sample.
 *
 *   path_smoke --errors                    device-free error codes only
 *   path_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD LAMPS.f32 KP AREA.f32 KA ALBEDO SKY BOUNCES OUT.bin
 *       SCENE.f32  N*9 float32 (file order); DIR.f32  KD bih_light; LAMPS.f32
 *       KP bih_point_light; AREA.f32  KA bih_area_light; renders frame FRAME of
 *       the W x H image (reference camera, seed 1984) with BOUNCES levels and
 *       writes, one after the other, lit (W*H*SPP u64), bounces (BOUNCES planes
 *       of W*H*SPP bih_hit), lits (BOUNCES planes of u64), irradiance, rgba
 *
 * Exit 0 = every check passed; prints one line per check.  Built by
 * tests/test_path.py with gcc -std=c11 -Wall -Wextra -Werror -pedantic
 * against -lbih_amd.
 */
#include "bih.h"

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(bih_path) == 5 * sizeof(void *) && offsetof(bih_path, bounces) == sizeof(void *) &&
                   offsetof(bih_path, lits) == 2 * sizeof(void *) && offsetof(bih_path, rgba) == 4 * sizeof(void *),
               "lit, bounces, lits, irradiance, rgba");
_Static_assert(BIH_MAX_BOUNCES == 8 && BIH_ABI_VERSION == 4, "constants");

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
                const bih_light_set *s, const bih_bounce *b, uint32_t nb, const bih_path *d, int expect) {
    return bih_render_path(t, c, w, h, spp, 0, 1984, rows, s, b, nb, d) == expect &&
           bih_render_path_device(t, c, w, h, spp, 0, 1984, rows, s, b, nb, d, NULL) == expect;
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
    const bih_path none = {NULL, NULL, NULL, NULL, NULL};
    bih_path rgba = none, hits = none, odd_lits = none, odd_hits = none;
    rgba.rgba = (uint32_t *)(void *)buf;
    hits.bounces = (bih_hit *)(void *)buf;
    odd_lits.lits = (uint64_t *)(void *)((char *)buf + 4);
    odd_hits.bounces = (bih_hit *)(void *)((char *)buf + 8);
    const bih_rows outside = {6, 4, 4, 1}, empty = {0, 0, 1, 1};
    const bih_light_set full = set_of(sun, 1, lamp, 1, pan, 1), zero = set_of(NULL, 0, NULL, 0, NULL, 0);
    const bih_light_set many = set_of(sun, 33, lamp, 31, pan, 1), a17 = set_of(NULL, 0, NULL, 0, pan, 17);
    const bih_light_set na = set_of(sun, 1, lamp, 1, NULL, 1);
    CHECK(both(NULL, &cam, 8, 8, 4, NULL, &full, &bn, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, NULL, 8, 8, 4, NULL, &full, &bn, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &full, &bn, 2, NULL, BIH_ERR_INVALID),
          "NULL tree, camera or planes -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 65, NULL, &full, &bn, 2, &rgba, BIH_ERR_INVALID), "spp > 64 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &full, &bn, 2, &none, BIH_ERR_INVALID), "all five planes NULL -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &outside, &full, &bn, 2, &rgba, BIH_ERR_INVALID), "bad rows -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &many, &bn, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &a17, &bn, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &na, &bn, 2, &rgba, BIH_ERR_INVALID),
          "too many lights, too many panels, a NULL array with a count -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &full, NULL, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, &bn, 0, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, &bn, BIH_MAX_BOUNCES + 1, &rgba, BIH_ERR_INVALID),
          "NULL bounce, n_bounces 0 or 9 -> INVALID (even with no rows)");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &full, &bn, 2, &odd_lits, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, &bn, 2, &odd_hits, BIH_ERR_INVALID),
          "misaligned lits or bounces -> INVALID (even with no rows)");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &full, &bn, 1, &hits, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, &zero, &bn, BIH_MAX_BOUNCES, &rgba, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, NULL, &bn, 3, &rgba, BIH_OK),
          "nrows == 0 -> OK; an empty or NULL light set is legal (sky only)");
    /* the level's direction: level 1 is bih_bounce_sample's, level 2 another; its checks */
    const float n[3] = {0.0f, 0.0f, 1.0f};
    float d[3] = {0.0f, 0.0f, 0.0f}, d1[3], d2[3];
    const int bad = bih_path_sample(1984, 0, 0, 4, 0, 1, NULL, d) == BIH_ERR_INVALID &&
                    bih_path_sample(1984, 0, 0, 4, 0, 1, n, NULL) == BIH_ERR_INVALID &&
                    bih_path_sample(1984, 0, 0, 0, 0, 1, n, d) == BIH_ERR_INVALID &&
                    bih_path_sample(1984, 0, 0, 4, 4, 1, n, d) == BIH_ERR_INVALID &&
                    bih_path_sample(1984, 0, 0, 4, 0, 0, n, d) == BIH_ERR_INVALID &&
                    bih_path_sample(1984, 0, 0, 4, 0, BIH_MAX_BOUNCES + 1, n, d) == BIH_ERR_INVALID;
    const int ok = bih_bounce_sample(1984, 5, 1, 4, 3, n, d) == BIH_OK &&
                   bih_path_sample(1984, 5, 1, 4, 3, 1, n, d1) == BIH_OK &&
                   bih_path_sample(1984, 5, 1, 4, 3, 2, n, d2) == BIH_OK;
    const float len2 = d2[0] * d2[0] + d2[1] * d2[1] + (d2[2] - 1.0f) * (d2[2] - 1.0f);
    CHECK(bad && ok && !memcmp(d, d1, sizeof d) && memcmp(d1, d2, sizeof d1) && len2 > 0.9999f && len2 < 1.0001f,
          "bih_path_sample: its checks; level 1 is bih_bounce_sample's, level 2 (%g, %g, %g) another", (double)d2[0],
          (double)d2[1], (double)d2[2]);
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--errors")) {
        check_errors();
        return g_fail;
    }
    if (argc != 17) {
        fprintf(stderr, "usage: path_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD LAMPS.f32 KP AREA.f32 KA ALBEDO SKY"
                        " BOUNCES OUT.bin | --errors\n");
        return 2;
    }
    const uint32_t n = (uint32_t)strtoul(argv[2], NULL, 10);
    const uint32_t w = (uint32_t)strtoul(argv[3], NULL, 10), h = (uint32_t)strtoul(argv[4], NULL, 10);
    const uint32_t spp = (uint32_t)strtoul(argv[5], NULL, 10), frame = (uint32_t)strtoul(argv[6], NULL, 10);
    const uint32_t kd = (uint32_t)strtoul(argv[8], NULL, 10), kp = (uint32_t)strtoul(argv[10], NULL, 10);
    const uint32_t ka = (uint32_t)strtoul(argv[12], NULL, 10);
    const bih_bounce bn = {strtof(argv[13], NULL), strtof(argv[14], NULL)};
    const uint32_t nb = (uint32_t)strtoul(argv[15], NULL, 10);
    const size_t P = (size_t)w * h, S = P * spp, L = S * nb;
    float *v = (float *)read_file(argv[1], (size_t)n * 9 * sizeof(float));
    bih_light *dir = (bih_light *)read_file(argv[7], (size_t)kd * sizeof(bih_light));
    bih_point_light *lamps = (bih_point_light *)read_file(argv[9], (size_t)kp * sizeof(bih_point_light));
    bih_area_light *area = (bih_area_light *)read_file(argv[11], (size_t)ka * sizeof(bih_area_light));
    bih_path d;
    d.lit = (uint64_t *)calloc(S ? S : 1, sizeof(uint64_t));
    d.bounces = (bih_hit *)calloc(L ? L : 1, sizeof(bih_hit));
    d.lits = (uint64_t *)calloc(L ? L : 1, sizeof(uint64_t));
    d.irradiance = (float *)calloc(P ? P : 1, sizeof(float));
    d.rgba = (uint32_t *)calloc(P ? P : 1, sizeof(uint32_t));
    if (!v || !dir || !lamps || !area || !d.lit || !d.bounces || !d.lits || !d.irradiance || !d.rgba) {
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
    rc = bih_render_path(tree, &cam, w, h, spp, frame, 1984, NULL, &set, &bn, nb, &d);
    CHECK(rc == BIH_OK, "bih_render_path %ux%ux%u frame %u, %u + %u + %u lights, %u bounces: %s", w, h, spp, frame, kd,
          kp, ka, nb, bih_strerror(rc));
    /* a path alive at level k was alive at level k-1; a lit word belongs to a stopped ray */
    size_t stopped = 0, bad = 0;
    for (uint32_t k = 0; k < nb; ++k)
        for (size_t i = 0; i < S; ++i) {
            const bih_hit *b = d.bounces + (size_t)k * S + i;
            const int hit = b->prim != BIH_NO_HIT;
            stopped += (size_t)hit;
            bad += (size_t)(d.lits[(size_t)k * S + i] != 0 && !hit) + (size_t)(hit && b->prim >= n);
            if (k > 0) bad += (size_t)(hit && d.bounces[(size_t)(k - 1) * S + i].prim == BIH_NO_HIT);
        }
    CHECK(bad == 0 && stopped > 0, "%zu stopped bounce rays over %u levels of %zu samples; %zu inconsistent records",
          stopped, nb, S, bad);
    bih_free(tree);

    FILE *f = fopen(argv[16], "wb");
    int wrote = f && fwrite(d.lit, 8, S, f) == S && fwrite(d.bounces, 16, L, f) == L && fwrite(d.lits, 8, L, f) == L &&
                fwrite(d.irradiance, 4, P, f) == P && fwrite(d.rgba, 4, P, f) == P;
    if (f) wrote = fclose(f) == 0 && wrote;
    CHECK(wrote, "planes written to %s", argv[16]);
    free(d.rgba); free(d.irradiance); free(d.lits); free(d.bounces); free(d.lit); free(area); free(lamps); free(dir);
    free(v);
    printf("%s\n", g_fail ? "path_smoke FAILED" : "path_smoke OK");
    return g_fail;
}
