// mlp_core.h -- what the fp32 MLP kernels share (forward: mlp_fp32.hip, mlp_fp32_wide.hip; backward-data: mlp_train.hip): the LDS weight
// ring fed by LDS-DMA, the register-resident GEMM part, accumulator <-> B-operand moves and the small VALU helpers; and the front end of
// the two forward kernels: their argument struct, its filler, the tile walk of a wave (RayTileWalk) and the launch plan behind it
// (walk_plan.h).  .hip translation units only.
#pragma once
#include "common.h"
#include "layout.h"
#include "walk_plan.h"

namespace minerf {

constexpr int NSLOT = 4;
constexpr int RING_BYTES = NSLOT * SLOT_BYTES;

// ---------------------------------------------------------------------------------------------
// front end of the forward kernels (mlp_fp32_kernel: 32-point wave tiles, mlp_fp32_wide_kernel: 16-point ones)
// ---------------------------------------------------------------------------------------------
struct MlpArgs : SideTables {  // stream_bytes: hoisted (MODE 0) or full (MODE 1) length, a multiple of SLOT_BYTES
    const float* rays;        // MODE 0: [n_rays, 6]
    const float* z;           // MODE 0: [n_rays, S]
    const float* x;           // MODE 1: [n_pts, in_x + in_d] with the NETWORK's own widths in_x = 3 + 6 Lx_net, in_d = 3 + 6 Ld_net
    int Lx_net, Ld_net;       // the network's frequencies (<= the kernel's LX / LD; the missing channels carry zero weights, layout.h)
    float* out;               // [n_pts, 4]
    long long n_wtiles;       // wave tiles
    long long n_pts;          // MODE 1
    // MODE 0 tile walk of one wave (walk_plan.h: tile_start, then tile_advance by these per step); n_iter steps for every wave
    long long n_rays, walk_ray, walk_carry, n_iter;
    int walk_chunk, ray_major;
    int S;                    // MODE 0
    int tpr;                  // MODE 0: wave tiles per ray = ceil(S / points per tile)
    unsigned long long* diag;  // MN_DIAG builds only: per-wave segment cycle sums + one tile's k-quad stamps
    // STASH kernels (training forward): row-major activations kept for the backward pass, P = stash_rows points
    float* stash_h;           // [D][P][W]   post-ReLU output of trunk layer l
    float* stash_f;           // [P][W]      linear_feat output
    float* stash_g;           // [P][W/2]    post-ReLU linear_d output
    unsigned* mask_h;         // [D][n_wtiles][64 lanes][4]  ReLU' bits of stash_h in the kernel's register order
    unsigned* mask_g;         // [n_wtiles][64 lanes][2]     ... of stash_g
    long long stash_rows;
};

static void fill_common(MlpArgs& a, const mi_nerf_net* net, const void* packed_dev, bool full_stream) {
    (SideTables&)a = side_tables(make_layout(net->D, net->W, net->skip, net->L_x, net->L_d), packed_dev, net->D, net->skip, full_stream);
    a.Lx_net = net->L_x; a.Ld_net = net->L_d;
}
// MODE 0: rays x their S depths in wave tiles of PTS points
template <int PTS>
static void fill_rays(MlpArgs& a, const float* rays_dev, const float* z_dev, int64_t n_rays, int S, float* raw_dev) {
    a.rays = rays_dev; a.z = z_dev; a.out = raw_dev; a.S = S; a.tpr = (S + PTS - 1) / PTS;
    a.n_wtiles = (long long)n_rays * a.tpr; a.n_rays = n_rays;
}

// What a launch needs beside its arguments: the LDS size (ring | side tables | per wave: the hoisted direction bias [W/2]), the opt-in for
// it, the grid (four wave tiles per workgroup) and the tile walk (MODE 1 walks flat: it has no rays).  opt_in: per kernel instantiation.
template <int W, int MODE>
static int plan_launch(MlpArgs& args, const void* kern, LdsOptIn& opt_in, size_t& lds, int& grid) {
    lds = RING_BYTES + (size_t)args.side_floats * 4 + 4 * (W / 2) * 4;
    MN_CHECK_ARG(lds <= 160 * 1024, "LDS budget exceeded: %zu bytes (a %d-deep network of width %d)", lds, args.D, W);
    if (int rc = ensure_lds_opt_in(opt_in, kern)) return rc;
    grid = persistent_grid((args.n_wtiles + 3) / 4);
    const long long tpr = MODE == 0 ? args.tpr : 1;
    const WalkPlan plan = walk_plan(args.n_rays, tpr, args.n_wtiles, grid, 4, MODE == 0);
    const TileStep step = tile_step(plan.ray_major, (long long)grid * 4, tpr);
    args.ray_major = plan.ray_major ? 1 : 0;
    args.n_iter = plan.n_iter;
    args.walk_ray = step.ray; args.walk_chunk = step.chunk; args.walk_carry = step.carry;
    return MI_NERF_OK;
}

// MODE 0: a wave's walk over its tiles of PTS points (lane column `col` < PTS owns one of them), the inputs of the NEXT tile (six ray
// scalars, one depth per lane) loaded a whole tile ahead.  No 64-bit division per tile: (ray, chunk) is stepped (walk_plan.h).  Per
// iteration: read this tile through ray() / chunk() / o / d / z, then advance() -- which issues the next tile's loads -- BEFORE building the
// point, so the loads have the whole tile to land.  A wave past the last ray recomputes the last tile (active() false: it stores nothing).
template <int PTS>
struct RayTileWalk {
    long long t_ray;
    int t_chunk;
    float o[3], d[3], z;
    __device__ __forceinline__ bool active(const MlpArgs& a) const { return t_ray < a.n_rays; }
    __device__ __forceinline__ long long ray(const MlpArgs& a) const { return active(a) ? t_ray : a.n_rays - 1; }
    __device__ __forceinline__ int chunk(const MlpArgs& a) const { return active(a) ? t_chunk : a.tpr - 1; }
    __device__ __forceinline__ void load(const MlpArgs& a, int col) {
        const long long r = ray(a);
        const int sample = chunk(a) * PTS + col;
        const int sc = sample < a.S ? sample : a.S - 1;
        const float* rp = a.rays + r * 6;
        o[0] = rp[0]; o[1] = rp[1]; o[2] = rp[2]; d[0] = rp[3]; d[1] = rp[4]; d[2] = rp[5];
        z = a.z[r * a.S + sc];
    }
    __device__ __forceinline__ void start(const MlpArgs& a, long long wid, int col) {
        tile_start(a.ray_major != 0, wid, a.tpr, t_ray, t_chunk);
        load(a, col);
    }
    __device__ __forceinline__ void advance(const MlpArgs& a, int col) {
        tile_advance(a.walk_ray, a.walk_chunk, a.walk_carry, a.tpr, t_ray, t_chunk);
        load(a, col);
    }
};

// ---------------------------------------------------------------------------------------------
// weight ring: NSLOT x 16 KiB in LDS, filled by LDS-DMA three slots ahead of the consumer.
//
// The DMA is issued from inline asm so that hipcc neither counts it (a counted DMA makes every
// __syncthreads() drain vmcnt(0), i.e. wait for the prefetch just issued) nor moves it; we count it
// ourselves: each ring_advance issues exactly 4 global_load_lds_dwordx4 per wave and waits vmcnt(4)
// before the barrier, i.e. for everything except the 4 issued at the previous advance.
//   advance to slot p: [vmcnt(4)] -> slots <= p+1 of this wave's share have landed; barrier -> of every
//   wave's share, and every wave has completed its LDS reads of slot p-1 (lgkmcnt(0) is part of the
//   barrier); then fetch slot p+3 into ring[(p+3)&3] == ring[(p-1)&3].
// Compiler-counted loads/stores elsewhere in the kernel only ever over-wait because of the uncounted DMA
// (vmcnt retires in order), never under-wait.
// ---------------------------------------------------------------------------------------------
struct WRing {
    const char* sbase;      // wave-uniform global pointer: stream + wave*4 KiB (the wave's quarter of every slot)
    unsigned voff;          // per-lane byte offset inside a quad: lane*16
    unsigned fetch_off;     // stream byte offset of the slot being fetched
    unsigned stream_bytes;
    unsigned fetch_lds;     // LDS byte address (wave-uniform) this wave's share of the next fetch lands at
    unsigned lds_lo, lds_hi;  // this wave's share of ring slot 0 / one past the last slot
    unsigned read_slot;     // ring slot being consumed
#ifdef MN_DIAG
    unsigned long long* dlog;   // fine-grained stamp log (one tile of one wave)
    unsigned dcnt;
#endif
};

#ifdef MN_DIAG
// diagnostic build only (never shipped, never timed): s_memtime stamps around the kernel's segments.  A stamp drains
// the LDS queue, so it perturbs what it measures (~100+ cycles each): read SHARES and DIFFERENCES, not totals.
__device__ __forceinline__ unsigned long long mn_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define MN_STAMP(i) do { const unsigned long long t_ = mn_stamp(); seg[i] += t_ - tprev; tprev = t_; } while (0)
#define MN_KQ_STAMP(ring) do { if ((ring).dlog && (ring).dcnt < 500) { (ring).dlog[(ring).dcnt] = mn_stamp(); (ring).dcnt++; } } while (0)
#else
#define MN_STAMP(i) do {} while (0)
#define MN_KQ_STAMP(ring) do {} while (0)
#endif

// one global_load_lds_dwordx4: 64 lanes x 16 B = one 1 KiB quad.  SGPR-base form: global address = sbase + voff + IMM,
// LDS destination = M0 + IMM + lane*16 (the instruction offset applies to BOTH sides).  M0 is compiler-reserved:
// saved and restored inside the statement.
template <int IMM>
__device__ __forceinline__ void dma16(const char* sbase, unsigned voff, unsigned lds_addr) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:%4\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(lds_addr), "i"(IMM)
        : "memory");
}

// DMA number I (0..3) of the slot being fetched
template <int I>
__device__ __forceinline__ void ring_dma(const WRing& r) {
    dma16<I * QUAD_BYTES>(r.sbase + r.fetch_off, r.voff, r.fetch_lds);
}

__device__ __forceinline__ void ring_next_fetch(WRing& r) {
    r.fetch_off += SLOT_BYTES;
    if (r.fetch_off >= r.stream_bytes) r.fetch_off = 0;
    r.fetch_lds += SLOT_BYTES;
    if (r.fetch_lds >= r.lds_hi) r.fetch_lds = r.lds_lo;
}

// Start consuming the next slot.  The four DMAs of a slot are NOT issued here in a burst (every extra issue slot
// between two MFMAs beyond ~8 delays the matrix pipe, tools/mfma_probe.hip): ring_read() issues DMA k together
// with the read of the slot's quad k+1, i.e. spread over the four groups that follow the barrier.
//
// ALLOW = operations that may still be in flight.  The slot being entered (p) is followed in the queue by the DMAs of
// slots p+1 and p+2 (4 each), so any ALLOW <= 8 is correct; 4 keeps one slot of slack (inference kernels).  The
// training kernels interleave one row store per k-quad with the DMAs (stores share vmcnt and retire in order): with
// ALLOW = 8 a store has one to two slot phases (4-8k cycles) to reach memory before an advance waits for it.
template <int ALLOW = 4>
__device__ __forceinline__ void ring_advance(WRing& r) {
    static_assert(ALLOW >= 0 && ALLOW <= 8, "more than 8 outstanding operations could include the entered slot's DMAs");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(ALLOW) : "memory");
    __syncthreads();
    ring_next_fetch(r);
    r.read_slot = (r.read_slot + 1) & (NSLOT - 1);
}

// qs is a compile-time constant at every call site once the GEMM loops are unrolled: the chain below folds away
__device__ __forceinline__ f32x4 ring_read(const char* smem, const WRing& r, int lane, int qs) {
    if (qs == 1) ring_dma<0>(r);
    else if (qs == 2) ring_dma<1>(r);
    else if (qs == 3) ring_dma<2>(r);
    else if (qs == 4) ring_dma<3>(r);
    return *(const f32x4*)(smem + r.read_slot * SLOT_BYTES + lane * 16 + qs * QUAD_BYTES);
}

// Start-up: a wave's view of the ring at the head of `stream` (smem: the ring's LDS), then slots 0..2 in bursts; from the first
// ring_advance on (the caller's: its barrier also publishes the caller's LDS tables) slot p+3 streams in, one DMA per group, while slot p
// is consumed.
__device__ __forceinline__ WRing ring_start(const char* stream, unsigned stream_bytes, const char* smem, int wave, int lane) {
    WRing r;
    r.sbase = stream + wave * (4 * QUAD_BYTES);
    r.voff = lane * 16;
    r.fetch_off = 0;
    r.stream_bytes = stream_bytes;
    r.lds_lo = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)smem + wave * (4 * QUAD_BYTES);
    r.lds_hi = r.lds_lo + RING_BYTES;
    r.fetch_lds = r.lds_lo;
    r.read_slot = NSLOT - 1;            // the first ring_advance moves to slot 0
#ifdef MN_DIAG
    r.dlog = nullptr; r.dcnt = 0;
#endif
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) {
        if (sl) ring_next_fetch(r);
        ring_dma<0>(r); ring_dma<1>(r); ring_dma<2>(r); ring_dma<3>(r);
    }
    return r;
}

// ---------------------------------------------------------------------------------------------
// one GEMM part: acc[0..NT) += A(stream) x B, B = KS per-lane registers b[0..KS).
// `a` is the A-operand pipeline: on entry it holds this part's quads (kq=0, t<NT), already read from
// LDS; after the 4 MFMAs that consume a[t] the quad NT positions further down the stream is read into
// it, so every LDS read has a full k-quad (NT*4 MFMAs) of lead time.  On exit `a` holds the first
// NT_NEXT quads of the NEXT part (parts are slot aligned, the stream is consumed strictly in order).
// MFMA order is t-major: 4 back-to-back dependent MFMAs per tile (dependent issue = 64 cycles = the
// issue interval of v_mfma_f32_32x32x2_f32, so the chain costs nothing).
// ---------------------------------------------------------------------------------------------
struct NoHook { __device__ __forceinline__ void operator()(int, int) const {} };

// `hook(kq, t)` runs inside the pinned group (kq, t) after its MFMAs and LDS read, with compile-time-constant
// arguments once the loops are unrolled: the training kernels use it to spread their row stores (and the ReLU-mask
// packing) over the GEMM that consumes the same registers, instead of a burst at the layer boundary that would block
// the texture-address path (shared by the 4 waves and by the weight DMAs) for ~9k cycles per layer.
template <int NT, int KS, int NT_NEXT, int ALLOW = 4, typename Hook = NoHook, int NB = 0>
__device__ __forceinline__ void gemm_part(f32x16 (&acc)[8], const float (&b)[NB], f32x4 (&a)[8], const char* smem,
                                          WRing& ring, int lane, Hook hook = Hook()) {
    static_assert(KS % 4 == 0 && KS <= NB, "k-steps come in quads");
    constexpr int KQ = KS / 4;
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][j], b[4 * kq + j], acc[t], 0, 0, 0);
            if (kq + 1 < KQ) {
                const int q = (kq + 1) * NT + t;                       // quad index inside this part
                if (q % SLOT_QUADS == 0) ring_advance<ALLOW>(ring);
                a[t] = ring_read(smem, ring, lane, q % SLOT_QUADS);
            } else if (t < NT_NEXT) {
                if (t == 0) ring_advance<ALLOW>(ring);                 // next part starts a fresh slot
                a[t] = ring_read(smem, ring, lane, t);
            }
            hook(kq, t);
            // pin the (4 MFMA, 1 LDS read) group order: left alone, hipcc sinks each read to just before
            // its first use and exposes the LDS latency on every tile
            __builtin_amdgcn_sched_barrier(0);
        }
        MN_KQ_STAMP(ring);
    }
#pragma unroll
    for (int t = NT; t < NT_NEXT; ++t) a[t] = ring_read(smem, ring, lane, t);
}

// acc tile t <- 32 floats of a natural-order vector in LDS (bias): register r of lane half hh holds
// feature 32t + (r&3) + 8*(r>>2) + 4*hh  -> four 16-byte reads at 32t + 8g + 4hh.
template <int NT>
__device__ __forceinline__ void acc_init(f32x16 (&acc)[8], const float* vec_lds, int hh) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = *(const f32x4*)(vec_lds + 32 * t + 8 * g + 4 * hh);
            acc[t][4 * g + 0] = v[0]; acc[t][4 * g + 1] = v[1]; acc[t][4 * g + 2] = v[2]; acc[t][4 * g + 3] = v[3];
        }
}

// ReLU as ONE instruction, pinned where it is written (volatile): gfx950's NaN-PROPAGATING maximum (v_maximum3_f32, IEEE 754-2019, as the
// split-precision kernel): negatives and -0.0 become +0.0, a NaN of EITHER sign stays a NaN.  (Until the far-point tests this was
// v_max_i32(bits, 0), which keeps +NaN but turns a NaN with its sign bit set -- 0 / 0 of a zero view direction, inf * 0 -- into 0: the
// network went on with zeros and returned plausible finite colours, tests/test_gpu_far_points.py.)  A plain fmaxf() costs two
// instructions (hipcc canonicalises the MFMA output first), returns the OTHER operand for a NaN, and hipcc defers it to directly in
// front of the MFMA that consumes the value, which then waits out the VALU latency plus hazard nops: ~20 cycles per k-step in the
// trunk layers (MN_DIAG stamps).
__device__ __forceinline__ float relu_pinned(float x) {
    float r;
    asm volatile("v_maximum3_f32 %0, %1, 0, 0" : "=v"(r) : "v"(x));
    return r;
}

template <int NT, bool RELU, int NB>
__device__ __forceinline__ void acc_to_b(const f32x16 (&acc)[8], float (&h)[NB]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) h[16 * t + r] = RELU ? relu_pinned(acc[t][r]) : acc[t][r];
}

// sum_i h[i] * w[feat(i, hh)] over this lane's half; w natural order in LDS
template <int N, int NB>
__device__ __forceinline__ float dot_half(const float (&h)[NB], const float* w_lds, int hh) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {        // q = 4t + g : features 32t + 8g + 4hh + {0..3}
        const f32x4 w = *(const f32x4*)(w_lds + 8 * q + 4 * hh);
        s0 = __builtin_fmaf(h[4 * q + 0], w[0], s0);
        s1 = __builtin_fmaf(h[4 * q + 1], w[1], s1);
        s2 = __builtin_fmaf(h[4 * q + 2], w[2], s2);
        s3 = __builtin_fmaf(h[4 * q + 3], w[3], s3);
    }
    return (s0 + s1) + (s2 + s3);
}

// row-major copy of a B-operand register set: registers 16t+4g..+3 of lane half hh are features 32t+8g+4hh+{0..3}
// of this lane's point -> one 16-byte store each.  `row` already includes the + 4*hh.
template <int NT, int NB>
__device__ __forceinline__ void store_rows(const float (&h)[NB], float* row, bool valid) {
    if (valid) {
#pragma unroll
        for (int q = 0; q < 4 * NT; ++q) {
            f32x4 v; v[0] = h[4 * q + 0]; v[1] = h[4 * q + 1]; v[2] = h[4 * q + 2]; v[3] = h[4 * q + 3];
            *(f32x4*)(row + 8 * q) = v;
        }
    }
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// chunk q (registers 4q..4q+3 = features 8q + 4hh + {0..3}) of a B-operand register set -> its row (one 16-byte store).
// Unconditional: an exec-masked store costs a saveexec/branch/restore triple inside the MFMA stream.  Callers make the
// padding lanes (sample >= S, inactive tail waves) recompute a VALID point, so their stores write the same bytes again.
template <int NB>
__device__ __forceinline__ void store_chunk(const float (&h)[NB], int q, float* row) {
    f32x4 v; v[0] = h[4 * q + 0]; v[1] = h[4 * q + 1]; v[2] = h[4 * q + 2]; v[3] = h[4 * q + 3];
    *(f32x4*)(row + 8 * q) = v;
}

// ReLU' bit masks.  Registers are packed in order, each word shifted left by one per value: register 4q+e lands in bit
// 31 - (4*(q&7)+e) of word q>>3 (words always fill: 8 chunks each).  The registers are post-ReLU (+0.0, positive or NaN,
// relu_pinned), so "non-zero bit pattern" == "> 0": min(bits, 1) shifted in, 2 VALU per value.  Pinned with asm volatile:
// written in C++, hipcc defers all 128 packs of a layer to the end of the GEMM (~2200 exposed cycles per layer).
template <int NB>
__device__ __forceinline__ void mask_bits_chunk(const float (&h)[NB], int q, unsigned (&bits)[4]) {   // 4 independent VALU
#pragma unroll
    for (int e = 0; e < 4; ++e) asm volatile("v_min_u32 %0, 1, %1" : "=v"(bits[e]) : "v"(h[4 * q + e]));
}
template <int NW>
__device__ __forceinline__ void mask_merge_chunk(const unsigned (&bits)[4], int q, unsigned (&mw)[NW]) {   // depth-3 tree, 4 VALU
    unsigned t01, t23;
    asm volatile("v_lshl_or_b32 %0, %1, 1, %2" : "=v"(t01) : "v"(bits[0]), "v"(bits[1]));
    asm volatile("v_lshl_or_b32 %0, %1, 1, %2" : "=v"(t23) : "v"(bits[2]), "v"(bits[3]));
    asm volatile("v_lshl_or_b32 %0, %1, 2, %2" : "=v"(t01) : "v"(t01), "v"(t23));
    asm volatile("v_lshl_or_b32 %0, %0, 4, %1" : "+v"(mw[q >> 3]) : "v"(t01));
}
template <int NB, int NW>
__device__ __forceinline__ void mask_pack_chunk(const float (&h)[NB], int q, unsigned (&mw)[NW]) {
    unsigned bits[4];
    mask_bits_chunk(h, q, bits);
    mask_merge_chunk(bits, q, mw);
}
// register 4q+e masked by its bit: extract the bit sign-extended (0 / ~0) and AND the float's bits -- two VALU per value, pinned:
// from the C++ shifts hipcc builds and + compare + select (three; VALU work beside fp32 MFMAs is paid in MFMA cycles).
template <int NW>
__device__ __forceinline__ float mask_apply(float v, int q, int e, const unsigned (&mw)[NW]) {
    int m;
    float r;
    asm volatile("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(mw[q >> 3]), "s"(31 - (4 * (q & 7) + e)));
    asm volatile("v_and_b32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(m));
    return r;
}

__device__ __forceinline__ float xhalf_sum(float v) { return v + __shfl_xor(v, 32, 64); }

}  // namespace minerf
