// Host program of tests/test_walk_plan_cpu.py: enumerates csrc/walk_plan.h (no device code, no HIP runtime).
//   walk_plan_enum n_rays units_per_ray grid waves [n_rays units_per_ray grid waves ...]
// Per case: "P <ray_major> <n_iter>", then per wave "U <wid> <unit of it = 0 .. n_iter - 1>" (the closed form, walk_unit) and
// "T <wid> <ray * units_per_ray + chunk per step>" (the fp32 kernels' incremental form: tile_start, tile_advance by tile_step).
#include <cstdio>
#include <cstdlib>
#include "walk_plan.h"

int main(int argc, char** argv) {
    using namespace minerf;
    for (int i = 1; i + 3 < argc; i += 4) {
        const long long n_rays = atoll(argv[i]), upr = atoll(argv[i + 1]);
        const int grid = atoi(argv[i + 2]), waves = atoi(argv[i + 3]);
        const long long NW = (long long)grid * waves;
        const WalkPlan plan = walk_plan(n_rays, upr, n_rays * upr, grid, waves);
        const TileStep step = tile_step(plan.ray_major, NW, upr);
        printf("P %d %lld\n", plan.ray_major ? 1 : 0, plan.n_iter);
        for (long long wid = 0; wid < NW; ++wid) {
            printf("U %lld", wid);
            for (long long it = 0; it < plan.n_iter; ++it)
                printf(" %u", walk_unit((unsigned)it, plan.ray_major ? (unsigned)upr : 0u, (unsigned)NW, (unsigned)wid));
            printf("\nT %lld", wid);
            long long ray;
            int chunk;
            tile_start(plan.ray_major, wid, (int)upr, ray, chunk);
            for (long long it = 0; it < plan.n_iter; ++it) {
                printf(" %lld", ray * upr + chunk);
                tile_advance(step.ray, step.chunk, step.carry, (int)upr, ray, chunk);
            }
            printf("\n");
        }
    }
    return 0;
}
