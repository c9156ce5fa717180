// row_slab.h -- "lattice rows as rays, then the fused network entry, then a reduction, slab by slab", written once for the two libraries
// that link against libmi_nerf.so and walk a lattice through a network: occ.hip (mi_occ_bake) and mesh.hip (mi_mesh_density).  Host code
// only, static / inline: neither library gains a symbol.  Like vox_rule.h's checks it has no error buffer and no words of its own: the
// including library passes its set_error, the subject of the sentence and the name of its *_scratch_bytes entry.
//
// A slab of R rows of S points is three regions of the caller's scratch, each rounded up to 256 bytes: rays [R,6], z [R,S], raw [R,S,4].
// The smallest scratch (what *_scratch_bytes answers) holds min_rows rows: min_points points, or the whole lattice.
#pragma once
#include <stdint.h>
#include "../../include/mi_nerf.h"
#include "abi_error.h"

namespace rowslab {

// the three fused entries share one signature
typedef int (*mlp_rays_fn)(const mi_nerf_net*, const void*, const float*, const float*, int64_t, int, float*, void*);

template <class Refuse>
static bool mlp_entry(Refuse refuse, const char* subject, int mode, mlp_rays_fn* fn) {
    switch (mode) {
        case MI_NERF_MODE_F32:  *fn = mi_nerf_mlp_rays; return true;
        case MI_NERF_MODE_F16S: *fn = mi_nerf_mlp_rays_f16s; return true;
        case MI_NERF_MODE_BF16: *fn = mi_nerf_mlp_rays_bf16; return true;
    }
    refuse("mode %d: %s runs MI_NERF_MODE_F32 (0), MI_NERF_MODE_BF16 (1) and MI_NERF_MODE_F16S (5)", mode, subject);
    return false;
}

static inline size_t slab_bytes(long long R, int S) { return align256((size_t)R * 24) + align256((size_t)R * S * 4) + align256((size_t)R * S * 16); }
static inline long long min_rows(long long rows, int S, long long min_points) {
    const long long want = (min_points + S - 1) / S;
    return want < rows ? want : rows;
}

struct Slab {
    long long rows, R;          // of the lattice; of a slab
    float *rays, *z, *raw;
};

// the scratch refusals, then the largest slab the scratch holds and its three pointers
template <class Refuse>
static bool plan(Refuse refuse, const char* bytes_entry, int S, long long rows, long long min_points, void* scratch, size_t scratch_bytes, Slab* out) {
    if (((uintptr_t)scratch & 255) != 0) return refuse("scratch must be 256-byte aligned"), false;
    const long long least = min_rows(rows, S, min_points);
    const size_t need = slab_bytes(least, S);
    if (scratch_bytes < need) return refuse("scratch too small: %zu < %zu (%s)", scratch_bytes, need, bytes_entry), false;
    long long R = (long long)((scratch_bytes - 768) / ((size_t)24 + (size_t)S * 20));
    if (R < least) R = least;                                            // fits: scratch_bytes >= need
    if (R > rows) R = rows;
    const long long r_cap = ((1LL << 31) - 1) / S;                       // a slab's R x S points stay below 2^31, the bound the render path keeps
    if (R > r_cap) R = r_cap;                                            // (min_points is far below it)
    char* w = (char*)scratch;
    *out = Slab{rows, R, (float*)w, (float*)(w + align256((size_t)R * 24)), (float*)(w + align256((size_t)R * 24) + align256((size_t)R * S * 4))};
    return true;
}

// the loop: slab(r0, nr) generates rows r0 .. r0 + nr into rays / z, calls the network into raw, reduces raw; it returns the library's
// status, and the first that is not 0 ends the walk
template <class OneSlab>
static int for_each(const Slab& s, OneSlab slab) {
    for (long long r0 = 0; r0 < s.rows; r0 += s.R)
        if (int rc = slab(r0, s.rows - r0 < s.R ? s.rows - r0 : s.R)) return rc;
    return 0;
}

}  // namespace rowslab
