/*
 * path_spec_smoke.c -- a plain C caller of the mirror path render of
 * include/bih.h (test infrastructure): bih_build, bih_tree_set_materials with
 * bih_material.kind, bih_camera_reference, bih_render_path_spec.
 *
 *   path_spec_smoke --errors                device-free error codes only
 *   path_spec_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD MAT.bin KM IDS.u32 SKY_R SKY_G SKY_B BOUNCES
 *       SCENE.f32  N*9 float32 (file order); DIR.f32  KD bih_light; MAT.bin  KM
 *       bih_material; IDS.u32  N uint32 (file order); renders frame FRAME of the
 *       W x H image (reference camera, seed 1984) with BOUNCES levels and prints
 *       "checksum %016llx": the sum, modulo 2^64, of (i + 1) * word_i over the
 *       32-bit words of lit, bounces, lits, radiance and rgba, one after the other
 *
 * Exit 0 = every check passed; prints one line per check.  Built by
 * tests/test_path_spec.py with gcc -std=c11 -Wall -Wextra -Werror -pedantic
 * against -lbih_amd.
 */
#include "bih.h"

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

_Static_assert(sizeof(bih_material) == 32 && offsetof(bih_material, emission) == 16, "albedo, emission: 16 bytes each");
_Static_assert(offsetof(bih_material, kind) == 12 && offsetof(bih_material, reserved0) == 12 &&
                   sizeof(((bih_material *)0)->kind) == 4 && BIH_MAT_DIFFUSE == 0u && BIH_MAT_MIRROR == 1u,
               "kind: the fourth word");
_Static_assert(sizeof(bih_path_rgb) == 5 * sizeof(void *) && offsetof(bih_path_rgb, bounces) == sizeof(void *) &&
                   offsetof(bih_path_rgb, lits) == 2 * sizeof(void *) &&
                   offsetof(bih_path_rgb, radiance) == 3 * sizeof(void *) &&
                   offsetof(bih_path_rgb, rgba) == 4 * sizeof(void *),
               "lit, bounces, lits, radiance, rgba");
_Static_assert(BIH_MAX_MATERIALS == 65536 && BIH_MAX_BOUNCES == 8 && BIH_ABI_VERSION == 4, "constants");

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
                const bih_light_set *s, const float *sky, uint32_t nb, const bih_path_rgb *d, int expect) {
    return bih_render_path_spec(t, c, w, h, spp, 0, 1984, rows, s, sky, nb, d) == expect &&
           bih_render_path_spec_device(t, c, w, h, spp, 0, 1984, rows, s, sky, nb, d, NULL) == expect;
}

/* The argument checks come before the tree is touched, so a stand-in tree
 * pointer (never dereferenced on these paths) reaches each of them. */
static void check_errors(void) {
    static _Alignas(16) float buf[16];
    static bih_camera cam;
    static bih_light sun[1] = {{{0.0f, 1.0f, 0.0f}, 1.0f}};
    static bih_point_light lamp[1] = {{{0.0f, 1.0f, 0.0f}, 1.0f}};
    static bih_area_light pan[1] = {{{0.0f, 1.0f, 0.0f}, 1.0f, {1.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 1.0f}, 0.0f}};
    static bih_material mirror[1] = {{{1.0f, 1.0f, 1.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f}};
    static const uint32_t ids[1] = {0};
    mirror[0].kind = BIH_MAT_MIRROR;
    const bih_tree *fake = (const bih_tree *)(const void *)buf;
    const float sky[3] = {0.25f, 0.3f, 0.4f};
    const bih_path_rgb none = {NULL, NULL, NULL, NULL, NULL};
    bih_path_rgb rgba = none, hits = none, odd_lits = none, odd_hits = none, odd_rad = none;
    rgba.rgba = (uint32_t *)(void *)buf;
    hits.bounces = (bih_hit *)(void *)buf;
    odd_lits.lits = (uint64_t *)(void *)((char *)buf + 4);
    odd_hits.bounces = (bih_hit *)(void *)((char *)buf + 8);
    odd_rad.radiance = buf + 1;
    const bih_rows outside = {6, 4, 4, 1}, empty = {0, 0, 1, 1};
    const bih_light_set full = set_of(sun, 1, lamp, 1, pan, 1), zero = set_of(NULL, 0, NULL, 0, NULL, 0);
    const bih_light_set many = set_of(sun, 33, lamp, 31, pan, 1), a17 = set_of(NULL, 0, NULL, 0, pan, 17);
    const bih_light_set na = set_of(sun, 1, lamp, 1, NULL, 1);
    CHECK(both(NULL, &cam, 8, 8, 4, NULL, &full, sky, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, NULL, 8, 8, 4, NULL, &full, sky, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &full, sky, 2, NULL, BIH_ERR_INVALID),
          "NULL tree, camera or planes -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 65, NULL, &full, sky, 2, &rgba, BIH_ERR_INVALID), "spp > 64 -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &full, sky, 2, &none, BIH_ERR_INVALID), "all five planes NULL -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &outside, &full, sky, 2, &rgba, BIH_ERR_INVALID), "bad rows -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, NULL, &many, sky, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &a17, sky, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, NULL, &na, sky, 2, &rgba, BIH_ERR_INVALID),
          "too many lights, too many panels, a NULL array with a count -> INVALID");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &full, NULL, 2, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, sky, 0, &rgba, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, sky, BIH_MAX_BOUNCES + 1, &rgba, BIH_ERR_INVALID),
          "NULL sky, n_bounces 0 or 9 -> INVALID (even with no rows)");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &full, sky, 2, &odd_lits, BIH_ERR_INVALID) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, sky, 2, &odd_hits, BIH_ERR_INVALID),
          "misaligned lits or bounces -> INVALID (even with no rows)");
    CHECK(both(fake, &cam, 8, 8, 4, &empty, &full, sky, 1, &hits, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, &full, sky, 1, &odd_rad, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, &zero, sky, BIH_MAX_BOUNCES, &rgba, BIH_OK) &&
              both(fake, &cam, 8, 8, 4, &empty, NULL, sky, 3, &rgba, BIH_OK),
          "nrows == 0 -> OK: the tree is never touched; radiance needs 4-byte alignment only");
    CHECK(bih_tree_set_materials(NULL, mirror, 1, ids) == BIH_ERR_INVALID &&
              bih_tree_set_materials(NULL, NULL, 0, NULL) == BIH_ERR_INVALID,
          "bih_tree_set_materials: NULL tree -> INVALID, a mirror in the palette or not");
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
    if (argc != 16) {
        fprintf(stderr, "usage: path_spec_smoke SCENE.f32 N W H SPP FRAME DIR.f32 KD MAT.bin KM IDS.u32 SKY_R SKY_G"
                        " SKY_B BOUNCES | --errors\n");
        return 2;
    }
    const uint32_t n = (uint32_t)strtoul(argv[2], NULL, 10);
    const uint32_t w = (uint32_t)strtoul(argv[3], NULL, 10), h = (uint32_t)strtoul(argv[4], NULL, 10);
    const uint32_t spp = (uint32_t)strtoul(argv[5], NULL, 10), frame = (uint32_t)strtoul(argv[6], NULL, 10);
    const uint32_t kd = (uint32_t)strtoul(argv[8], NULL, 10), km = (uint32_t)strtoul(argv[10], NULL, 10);
    const float sky[3] = {strtof(argv[12], NULL), strtof(argv[13], NULL), strtof(argv[14], NULL)};
    const uint32_t nb = (uint32_t)strtoul(argv[15], NULL, 10);
    const size_t P = (size_t)w * h, S = P * spp, L = S * nb;
    float *v = (float *)read_file(argv[1], (size_t)n * 9 * sizeof(float));
    bih_light *dir = (bih_light *)read_file(argv[7], (size_t)kd * sizeof(bih_light));
    bih_material *mat = (bih_material *)read_file(argv[9], (size_t)km * sizeof(bih_material));
    uint32_t *ids = (uint32_t *)read_file(argv[11], (size_t)n * sizeof(uint32_t));
    bih_path_rgb d;
    d.lit = (uint64_t *)calloc(S ? S : 1, sizeof(uint64_t));
    d.bounces = (bih_hit *)calloc(L ? L : 1, sizeof(bih_hit));
    d.lits = (uint64_t *)calloc(L ? L : 1, sizeof(uint64_t));
    d.radiance = (float *)calloc(P ? 3 * P : 1, sizeof(float));
    d.rgba = (uint32_t *)calloc(P ? P : 1, sizeof(uint32_t));
    if (!v || !dir || !mat || !ids || !d.lit || !d.bounces || !d.lits || !d.radiance || !d.rgba) {
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
    const bih_light_set set = set_of(kd ? dir : NULL, kd, NULL, 0, NULL, 0);
    rc = bih_render_path_spec(tree, &cam, w, h, spp, frame, 1984, NULL, &set, sky, nb, &d);
    CHECK(rc == BIH_ERR_INVALID, "bih_render_path_spec on a tree without materials: %s", bih_strerror(rc));
    /* a kind that is neither DIFFUSE nor MIRROR: the set is accepted, the colour call renders it, this call does not */
    uint32_t mirrors = 0;
    for (uint32_t k = 0; k < km; ++k) mirrors += (uint32_t)(mat[k].kind == BIH_MAT_MIRROR);
    const uint32_t kind0 = mat[0].kind;
    mat[0].kind = 2u;
    rc = bih_tree_set_materials(tree, mat, km, ids);
    CHECK(rc == BIH_OK && bih_render_path_spec(tree, &cam, w, h, spp, frame, 1984, NULL, &set, sky, nb, &d) ==
                              BIH_ERR_INVALID &&
              bih_render_path_rgb(tree, &cam, w, h, spp, frame, 1984, NULL, &set, sky, nb, &d) == BIH_OK,
          "a palette with kind 2: bih_render_path_spec INVALID, bih_render_path_rgb OK");
    mat[0].kind = kind0;
    rc = bih_tree_set_materials(tree, mat, km, ids);
    CHECK(rc == BIH_OK && mirrors > 0, "bih_tree_set_materials, %u materials, %u of them mirrors: %s", km, mirrors,
          bih_strerror(rc));
    /* the colour call on the same set, for comparison: it ignores the kinds */
    float *diffuse = (float *)calloc(P ? 3 * P : 1, sizeof(float));
    bih_path_rgb only = {NULL, NULL, NULL, NULL, NULL};
    only.radiance = diffuse;
    rc = diffuse ? bih_render_path_rgb(tree, &cam, w, h, spp, frame, 1984, NULL, &set, sky, nb, &only) : BIH_ERR_OOM;
    CHECK(rc == BIH_OK, "bih_render_path_rgb, radiance only: %s", bih_strerror(rc));
    rc = bih_render_path_spec(tree, &cam, w, h, spp, frame, 1984, NULL, &set, sky, nb, &d);
    CHECK(rc == BIH_OK, "bih_render_path_spec %ux%ux%u frame %u, %u lights, %u bounces: %s", w, h, spp, frame, kd, nb,
          bih_strerror(rc));
    size_t differ = 0;
    for (size_t p = 0; diffuse && p < 3 * P; ++p) differ += (size_t)(memcmp(diffuse + p, d.radiance + p, 4) != 0);
    CHECK(differ > 0, "%zu of %zu radiance values differ from the colour call's: the mirrors steer", differ, 3 * P);
    free(diffuse);
    bih_free(tree);

    uint64_t sum = 0, i = 0;
    sum = fold(sum, &i, d.lit, S * 8);
    sum = fold(sum, &i, d.bounces, L * 16);
    sum = fold(sum, &i, d.lits, L * 8);
    sum = fold(sum, &i, d.radiance, P * 12);
    sum = fold(sum, &i, d.rgba, P * 4);
    printf("checksum %016llx\n", (unsigned long long)sum);
    free(d.rgba); free(d.radiance); free(d.lits); free(d.bounces); free(d.lit); free(ids); free(mat); free(dir);
    free(v);
    printf("%s\n", g_fail ? "path_spec_smoke FAILED" : "path_spec_smoke OK");
    return g_fail;
}
