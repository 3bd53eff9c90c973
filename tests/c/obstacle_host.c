/* obstacle_host.c -- csrc/obstacle_math.inc compiled for the host (the text the kernels of gpd_obstacles compile), evaluated on a
 * scene the test hands over: every signed distance with its gradient and every ray entry, then the reductions of the two kernels
 * (the minimum, ties to the lower record; ranges capped at max_range).  tests/test_host_obstacles.py compares what it writes with the
 * float64 restatement.  Runs under AddressSanitizer + UndefinedBehaviorSanitizer.
 *   obstacle_host IN OUT
 *   IN : int32 M, N, R; float32 max_range, collision_radius; obst [M][8]; pos [N][3]; dirs [N][R][3]
 *   OUT: float32 d [N][M], grad [N][M][3], t [N][M][R], clear4 [N][4], ranges [N][R]; int32 nearest [N], hit [N], ray_hit [N][R] */
#include <stdio.h>
#include <stdlib.h>

#include "gpd.h"
#include "obstacle_math.inc"

static void* need(size_t count, size_t size) {
    void* p = calloc(count ? count : 1, size);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: obstacle_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int32_t dims[3];
    float scal[2];
    if (fread(dims, sizeof(int32_t), 3, in) != 3 || fread(scal, sizeof(float), 2, in) != 2) { fprintf(stderr, "short header\n"); return 2; }
    const int M = dims[0], N = dims[1], R = dims[2];
    const float max_range = scal[0], collision_radius = scal[1];
    if (M < 1 || M > GPD_OBST_MAX || N < 1 || N > 100000 || R < 1 || R > GPD_OBST_MAX_RAYS) { fprintf(stderr, "bad sizes\n"); return 2; }
    float* obst = need((size_t)M * GPD_OBST_FLOATS, sizeof(float));
    float* pos = need((size_t)N * 3, sizeof(float));
    float* dirs = need((size_t)N * R * 3, sizeof(float));
    if (fread(obst, sizeof(float), (size_t)M * GPD_OBST_FLOATS, in) != (size_t)M * GPD_OBST_FLOATS || fread(pos, sizeof(float), (size_t)N * 3, in) != (size_t)N * 3 ||
        fread(dirs, sizeof(float), (size_t)N * R * 3, in) != (size_t)N * R * 3) { fprintf(stderr, "short input\n"); return 2; }
    fclose(in);
    float* d = need((size_t)N * M, sizeof(float));
    float* grad = need((size_t)N * M * 3, sizeof(float));
    float* t = need((size_t)N * M * R, sizeof(float));
    float* clear4 = need((size_t)N * 4, sizeof(float));
    float* ranges = need((size_t)N * R, sizeof(float));
    int32_t* nearest = need((size_t)N, sizeof(int32_t));
    int32_t* hit = need((size_t)N, sizeof(int32_t));
    int32_t* ray_hit = need((size_t)N * R, sizeof(int32_t));
    for (int i = 0; i < N; ++i) {
        const float* p = pos + 3 * i;
        float best = GPD_OBST_INF, bn[3] = {0.0f, 0.0f, 0.0f};
        int who = -1;
        for (int r = 0; r < R; ++r) { ranges[(size_t)i * R + r] = max_range; ray_hit[(size_t)i * R + r] = -1; }
        for (int m = 0; m < M; ++m) {
            const float* o = obst + (size_t)m * GPD_OBST_FLOATS;
            const int kind = (int)o[3];
            const float vx = p[0] - o[0], vy = p[1] - o[1], vz = p[2] - o[2];
            float* g = grad + ((size_t)i * M + m) * 3;
            const float dm = gpd_obst_sdf(kind, o[4], o[5], o[6], vx, vy, vz, &g[0], &g[1], &g[2]);
            d[(size_t)i * M + m] = dm;
            if (dm < best) { best = dm; who = m; bn[0] = g[0]; bn[1] = g[1]; bn[2] = g[2]; }
            for (int r = 0; r < R; ++r) {
                const float* u = dirs + ((size_t)i * R + r) * 3;
                const float tm = gpd_obst_ray(kind, o[4], o[5], o[6], vx, vy, vz, u[0], u[1], u[2]);
                t[((size_t)i * M + m) * R + r] = tm;
                if (tm < ranges[(size_t)i * R + r]) { ranges[(size_t)i * R + r] = tm; ray_hit[(size_t)i * R + r] = m; }
            }
        }
        clear4[4 * i] = bn[0]; clear4[4 * i + 1] = bn[1]; clear4[4 * i + 2] = bn[2]; clear4[4 * i + 3] = best;
        nearest[i] = who;
        hit[i] = best < collision_radius;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    size_t ok = fwrite(d, sizeof(float), (size_t)N * M, out) + fwrite(grad, sizeof(float), (size_t)N * M * 3, out) +
                fwrite(t, sizeof(float), (size_t)N * M * R, out) + fwrite(clear4, sizeof(float), (size_t)N * 4, out) +
                fwrite(ranges, sizeof(float), (size_t)N * R, out) + fwrite(nearest, sizeof(int32_t), (size_t)N, out) +
                fwrite(hit, sizeof(int32_t), (size_t)N, out) + fwrite(ray_hit, sizeof(int32_t), (size_t)N * R, out);
    const size_t want = (size_t)N * M * (4 + R) + (size_t)N * (4 + R + 2 + R);
    if (fclose(out) != 0 || ok != want) { fprintf(stderr, "short write\n"); return 2; }
    free(obst); free(pos); free(dirs); free(d); free(grad); free(t); free(clear4); free(ranges); free(nearest); free(hit); free(ray_hit);
    printf("obstacle_host: %d drones x %d obstacles x %d rays\n", N, M, R);
    return 0;
}
