// walk_plan.h -- how the persistent MLP kernels deal a launch's units of work to their waves: the one decision "whole rays per wave, or a
// flat walk" (host), the closed form of the resulting walk (host and device), and the incremental form the fp32 kernels step through.
// Integer arithmetic only and no device or runtime call: it compiles with a plain host compiler (tests/test_walk_plan_cpu.py enumerates it).
//
// A launch covers n_units units (a unit = what one wave computes per iteration: one or two point tiles) with NW = grid x waves_per_group
// waves; every wave runs the same n_iter iterations (the weight ring's barriers are workgroup-wide), inactive ones recompute the last unit.
//   flat:       iteration `it` of wave `wid` takes unit it * NW + wid;
//   ray-major:  a wave takes whole rays (ray wid, wid + NW, ...) and their units_per_ray units back to back, so the per-ray work of the
//               prologue (the view-direction encoding and its hoisted linear_d term) is done once per ray instead of once per unit.
#pragma once

#if defined(__HIP__) || defined(__CUDACC__)
#define MN_WALK_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define MN_WALK_FN inline __attribute__((always_inline))
#endif

namespace minerf {

struct WalkPlan {
    bool ray_major;
    long long n_iter;       // iterations of every wave
};

// Ray-major once every wave of the grid gets at least one whole ray, and dealing whole rays does not cost a round more than dealing units
// (1500 rays x 6 tiles on 1024 waves: 12 steps ray-major, 9 flat).  rays_whole: the launch may deal whole rays at all (it reads rays, it
// starts at a ray's first unit, a ray is a whole number of units) -- the caller's own conditions.
MN_WALK_FN WalkPlan walk_plan(long long n_rays, long long units_per_ray, long long n_units, int grid, int waves_per_group, bool rays_whole = true) {
    const long long NW = (long long)grid * waves_per_group;
    const long long it_ray = (n_rays + NW - 1) / NW * units_per_ray, it_flat = (n_units + NW - 1) / NW;
    const bool ray_major = rays_whole && n_rays >= NW && it_ray <= it_flat;
    return WalkPlan{ray_major, ray_major ? it_ray : it_flat};
}

// the unit of iteration `it` on wave `wid` of NW; ppr = units per ray on the ray-major walk, 0 on the flat one
MN_WALK_FN unsigned walk_unit(unsigned it, unsigned ppr, unsigned NW, unsigned wid) {
    if (ppr) { const unsigned blk = it / ppr; return (blk * NW + wid) * ppr + (it - blk * ppr); }
    return it * NW + wid;
}

// The same walk without a division per step (the fp32 kernels: tile = (ray, chunk), tpr chunks per ray).  A wave starts at tile_start()
// and adds (ray, chunk) per step; a chunk overflow carries `carry` rays.
struct TileStep {
    long long ray, carry;
    int chunk;
};
MN_WALK_FN TileStep tile_step(bool ray_major, long long NW, long long tpr) {
    if (ray_major) return TileStep{0, NW, 1};
    return TileStep{NW / tpr, 1, (int)(NW % tpr)};
}
MN_WALK_FN void tile_start(bool ray_major, long long wid, int tpr, long long& ray, int& chunk) {
    if (ray_major) { ray = wid; chunk = 0; }
    else { ray = wid / tpr; chunk = (int)(wid - ray * tpr); }
}
MN_WALK_FN void tile_advance(long long step_ray, int step_chunk, long long step_carry, int tpr, long long& ray, int& chunk) {
    ray += step_ray;
    chunk += step_chunk;
    if (chunk >= tpr) { chunk -= tpr; ray += step_carry; }
}

}  // namespace minerf
