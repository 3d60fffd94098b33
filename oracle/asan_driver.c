/* oracle/asan_driver.c -- runs the C restatement under AddressSanitizer + UBSan (CPU only; GPU
 * sanitizers are not available on the pool).  Built and run by tests/test_oracle_sanitizers.py.
 * TEST INFRASTRUCTURE ONLY. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssd_oracle.h"

static const char *HARVEST[] = {"@@@@@@@@", "@P A AP@", "@ AAA  @", "@PA  AP@", "@  A   @", "@P AA P@", "@@@@@@@@"};
static const char *CLEANUP[] = {"@@@@@@@@", "@HRP BB@", "@RH PBB@", "@HHSSBP@", "@RRP BB@", "@HR  PB@", "@@@@@@@@"};

/* tables: 0 = the reference's constants; 1 = caller-supplied spawn tables (ssd_oracle_set_tables): thresholds of 0, 2^32 and above
 * and draw-decided ones, set, taken back and set again. */
static int run(int game, const char **rows, int H, int W, int E, int N, int tables) {
    char *map = (char *)malloc((size_t)H * W);
    for (int r = 0; r < H; ++r) memcpy(map + (size_t)r * W, rows[r], (size_t)W);
    uint8_t lut[128 * 3];
    for (int i = 0; i < 128 * 3; ++i) lut[i] = (uint8_t)(i * 7);
    ssd_oracle *o = ssd_oracle_create(game, H, W, map, E, N, 7, 5, 12345u, 3u, lut);
    if (!o) return 1;
    uint32_t *waste = (uint32_t *)malloc(sizeof(uint32_t) * E);
    if (tables) {
        const uint64_t harvest[4] = {1ull << 26, 1ull << 32, 0, 1ull << 40};
        const int n = ssd_oracle_potential_waste_area(o) + 1;
        uint64_t *ca = (uint64_t *)malloc(sizeof(uint64_t) * n), *cw = (uint64_t *)malloc(sizeof(uint64_t) * n);
        for (int i = 0; i < n; ++i) {
            ca[i] = i % 2 ? 0 : (i % 4 ? 1ull << 63 : 1ull << 31);
            cw[i] = i % 3 ? 1ull << 32 : 0;
        }
        if (ssd_oracle_set_tables(o, harvest, ca, NULL) == 0) return 6;    /* one Cleanup table without the other: rejected */
        if (ssd_oracle_set_tables(o, harvest, ca, cw)) return 6;
        if (ssd_oracle_set_tables(o, NULL, NULL, NULL)) return 6;
        if (ssd_oracle_set_tables(o, harvest, ca, cw)) return 6;
        free(ca); free(cw);
    }
    const int V = 15;
    uint8_t *obs = (uint8_t *)malloc((size_t)E * N * V * V * 3);
    int32_t *rew = (int32_t *)malloc(sizeof(int32_t) * E * N), *act = (int32_t *)malloc(sizeof(int32_t) * E * N);
    uint8_t *done = (uint8_t *)malloc((size_t)E * N), *mask = (uint8_t *)malloc((size_t)E);
    long total = 0;
    if (ssd_oracle_reset(o, NULL, obs)) return 2;
    for (int s = 0; s < 400; ++s) {
        if (ssd_oracle_step_random(o, game == 0 ? 8 : 9, act, obs, rew, done)) return 3;
        for (int i = 0; i < E * N; ++i) total += rew[i];
        if (ssd_oracle_get_waste_count(o, waste)) return 7;
        for (int e = 0; e < E; ++e) total += waste[e] & 1u;
        if (s % 50 == 49) {
            for (int e = 0; e < E; ++e) mask[e] = (uint8_t)((e + s) & 1);
            if (ssd_oracle_reset(o, mask, obs)) return 4;
        }
    }
    if (ssd_oracle_observe(o, 0, obs)) return 5;
    printf("game %d%s ok, checksum %ld\n", game, tables ? " with tables" : "", total);
    free(waste);
    free(map); free(obs); free(rew); free(act); free(done); free(mask);
    ssd_oracle_destroy(o);
    return 0;
}

int main(void) {
    int rc = run(0, HARVEST, 7, 8, 16, 6, 0);
    if (rc) return rc;
    if ((rc = run(1, CLEANUP, 7, 8, 16, 5, 0))) return rc;
    if ((rc = run(0, HARVEST, 7, 8, 16, 6, 1))) return rc;
    return run(1, CLEANUP, 7, 8, 16, 5, 1);
}
