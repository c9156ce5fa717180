// mlp_half_core.h -- the one-MFMA-per-product kernel shared by the bf16 (mlp_bf16.hip) and f16 (mlp_f16.hip) variants: constants, the
// fragment file, packing schedule, job(), the forward kernel body, its launcher and launch plan (the weight ring and the MFMA wrappers:
// wstream_ring.h; the ray-major / flat decision and the walk's closed form: walk_plan.h; the f16 point encoder and the hoisted
// view-direction term: common.h; the side-table record at the head of the arguments: layout.h).  The element type is a template parameter (F16) decided with `if constexpr`; see mlp_bf16.hip for the design and
// mlp_f16.hip for what the f16 instantiation changes.
#pragma once
#include "wstream_ring.h"
#include "stage_dev.h"

namespace minerf {

// where the next unit's inputs are requested in the view-direction layer: (job, k-step)
constexpr int BF16_PF_T = 3, BF16_PF_KS = 2;

// Point tiles (16 points each) per wave: 4 in the standard shape (64 points per wave, 256 per workgroup and pass of the weight
// stream), 2 in the SMALL-LAUNCH shape (32 / 128): twice the LDS reads and weight stream per FLOP, chosen by the launcher only
// where the 64-point shape would leave SIMDs idle (a 512-ray shard of BASELINE config #5's 8-GPU split: 128 + 384 workgroup
// passes on 256 CUs become 256 + 768 half-size ones).  NP is a template parameter of everything below.
// (MT = 16 output features per job, KF = 32 k per MFMA, the tail's TAIL_USED of TAIL_QUADS positions and enc_ksteps32: half_layout.h)
constexpr int DA = 4;                                      // A-operand pipeline depth (fragments in flight)
// (the ring: HSLOT_QUADS = 32 quads per slot, HNSLOT = 3 slots, hring_dmas(NWV) DMAs per wave and slot: wstream_ring.h)

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
struct PhaseB {
    unsigned tile0, tile_end;   // this phase's range of 32-point tiles; tiles are numbered ray * tpr + chunk over the whole call
    unsigned n_iter;            // units per wave (the same for every wave: the ring barriers are workgroup-wide); a unit = NP / 2 tiles
    unsigned ppr;               // ray-major walk: units per ray (tpr / (NP / 2)); 0: flat walk
};
struct MlpArgsB : SideTables {  // (layout.h; filled by half_layout.h's side_tables)
    const float* rays;
    const float* z;             // [n_rays, S] depths; NULL: the coarse pass draws its own stratified depths (strat_*) and writes them to z_out
    float* z_out;
    float strat_near, strat_far, strat_step;
    Jitter strat_jitter;
    float* out;
    PhaseB ph[2];               // one or two phases (see run_phase); the kernel's template arguments say how many and of which shape
    unsigned n_rays;
    int S, tpr;
    unsigned long long* diag;   // MN_DIAG builds only: per-wave cycle sums of the kernel's segments
    // small coarse launches (one 32-point unit per wave, two units per ray: a workgroup's four waves hold rays 2b and 2b + 1 whole): the
    // workgroup composites its two rays and draws their fine depths in the kernel's epilogue (stage_dev.h), fz_on != 0
    int fz_on, fz_Nf, fz_n2, fz_det;
    Jitter fz_u;
    float *fz_rgb, *fz_disp, *fz_w, *fz_zf;
};

#ifdef MN_DIAG
// diagnostic build only (never shipped, never timed): s_memtime stamps around the kernel's segments (read SHARES, not totals)
__device__ __forceinline__ unsigned long long bstamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define BSTAMP(i) do { const unsigned long long t_ = bstamp(); seg[i] += t_ - tprev; tprev = t_; } while (0)
#else
#define BSTAMP(i) do {} while (0)
#endif

// ELEMENT TYPE.  Every template below takes `bool F16`: false = bf16 operands (mlp_bf16.hip), true = f16 operands (mlp_f16.hip) read from
// the split-precision blob; what that means for the weight stream is written at the ring (wstream_ring.h).

// two floats -> one dword of a B fragment (round to nearest even).  Pinned where it is written.
// f16: a value at or beyond 65520 converts to +-inf; h * 0 + h turns that into NaN (finite h: h exactly) before anything can clamp it
// (the RANGE CONTRACT of the split-precision mode, mlp_f16s_core.h, include/mi_nerf.h).
template <bool F16>
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    unsigned d;
    if constexpr (F16) asm volatile("v_cvt_pk_f16_f32 %0, %1, %2\n\tv_pk_fma_f16 %0, %0, 0, %0" : "=&v"(d) : "v"(lo), "v"(hi));
    else asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(d) : "v"(lo), "v"(hi));
    return d;
}

// ---------------------------------------------------------------------------------------------
// THE FRAGMENT FILE: all 256 AGPRs, managed by hand.
//
// Two sets (ping-pong between consecutive layers) x NP point tiles x 8 B fragments x 4 registers = 256 (NP = 4) = the whole
// accumulation-register file (half of it at NP = 2).  With most of the wave's 512 registers live, hipcc's allocator could not place these tuples
// (it treats MFMA operands as "either file" values and thrashed: fragments copied AGPR -> VGPR in front of every MFMA,
// accumulators spilled around the packing, up to 300 spilled registers) -- so the fragments never become compiler values at
// all: they are written with v_accvgpr_write_b32 a[N] and read as the MFMA's B operand a[N:N+3] with N a compile-time
// constant, and the compiler allocates only the VGPR side.  It must keep out of the AGPRs entirely: this file is built with
// -mllvm -amdgpu-spill-vgpr-to-agpr=0 and contains no MFMA builtin; one clobber of a255 makes the kernel descriptor reserve
// the whole file (tests/test_packing_cpu.py checks the object).
//
// Consequence: the MFMAs are asm statements and hipcc inserts NO hazard wait states around them.  They hold by construction:
//   * the four accumulation chains of a job are interleaved, a chain's next MFMA is four issues (64 cycles) behind;
//   * every other reader of an MFMA result (the packing of a finished tile, the final store) is at least four MFMA issues
//     behind the MFMA that wrote it -- the packing starts in the NEXT job's second group, the store and the density read-out
//     are preceded by whole groups / explicit s_nops;
//   * a fragment register is written at least one whole group (>= 64 cycles) before the MFMA that reads it and never while an
//     MFMA that reads it can be in flight (a layer writes the OTHER set; the half fragment packed across a layer boundary is
//     the last one that layer reads);
//   * the C operand of a job's first MFMAs is kept allocated until the next group (the matrix pipe reads it after issue);
//   * VGPR operands (A fragments, biases, gamma(x)) come from LDS reads the compiler tracks (s_waitcnt before the asm).
// ---------------------------------------------------------------------------------------------
// (the MFMA wrappers themselves -- mfma_first<F16>: a job's first MFMA, C operand = the bias; mfma_acc<F16>: accumulate -- are wstream_ring.h's)
__host__ __device__ constexpr int frag_reg(int np, int set, int p, int f) { return ((set * np + p) * 8 + f) * 4; }

// A finished 16x16 tile (4 accumulator registers per lane) -> two packed dwords -> registers R, R + 1 of the fragment file
// (tile t of a layer is dwords 2(t&1), 2(t&1)+1 of fragment t>>1).  ReLU on the packed pair, one instruction per dword.  bf16: the
// NaN-propagating f16 maximum v_pk_maximum3_f16 on the bf16 BIT PATTERNS -- the sign bit is the same bit, so every negative bf16 (and
// -0.0) reads as a negative f16 and becomes +0, every non-negative one is returned unchanged, and a bf16 NaN of either sign reads as a
// QUIET f16 NaN (bits 14..7 set, bit 9 among them) and is returned unchanged.  (v_pk_max_i16, used until the far-point tests, turned a
// NaN with its sign bit set into 0 and the network returned finite colours for NaN inputs.)  Two patterns differ from the integer
// maximum: bf16 -inf reads as an f16 NaN and STAYS -inf (the next layer turns it into inf / NaN instead of treating the unit as off), and
// |x| >= 2^121 with bit 9 clear reads as a signalling f16 NaN and is quieted (another value of that size); neither occurs for finite
// inputs.  In three stages of two independent instructions each, one stage per MFMA gap (a 16-cycle
// MFMA leaves room for two VALU issues), or as one statement where there are more gaps than work.
// f16 (stage 1 carries two or four instructions): the ReLU as gfx950's NaN-PROPAGATING maximum (v_pk_maximum3_f16, as the split-precision
// kernel), then +-inf -> NaN as in pack2.  In that order a pre-activation
// <= -65520 in front of a ReLU is an exact 0 (the unit is off, as in fp32) and +inf, or -inf out of linear_feat (no ReLU), is NaN.
template <bool F16, bool RELU, int R, int STAGE>
__device__ __forceinline__ void pack_stage(const f32x4& acc, unsigned (&t)[2]) {
    if constexpr (F16) {
        if constexpr (STAGE == 0) asm volatile("v_cvt_pk_f16_f32 %0, %2, %3\n\tv_cvt_pk_f16_f32 %1, %4, %5" : "=&v"(t[0]), "=&v"(t[1]) : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]));
        else if constexpr (STAGE == 1) {
            if (RELU) asm volatile("v_pk_maximum3_f16 %0, %0, 0, 0\n\tv_pk_maximum3_f16 %1, %1, 0, 0" : "+v"(t[0]), "+v"(t[1]));
            asm volatile("v_pk_fma_f16 %0, %0, 0, %0\n\tv_pk_fma_f16 %1, %1, 0, %1" : "+v"(t[0]), "+v"(t[1]));
        }
        else asm volatile("v_accvgpr_write_b32 a[%2], %0\n\tv_accvgpr_write_b32 a[%3], %1" ::"v"(t[0]), "v"(t[1]), "n"(R), "n"(R + 1));
    } else {
        if constexpr (STAGE == 0) asm volatile("v_cvt_pk_bf16_f32 %0, %2, %3\n\tv_cvt_pk_bf16_f32 %1, %4, %5" : "=&v"(t[0]), "=&v"(t[1]) : "v"(acc[0]), "v"(acc[1]), "v"(acc[2]), "v"(acc[3]));
        else if constexpr (STAGE == 1) { if (RELU) asm volatile("v_pk_maximum3_f16 %0, %0, 0, 0\n\tv_pk_maximum3_f16 %1, %1, 0, 0" : "+v"(t[0]), "+v"(t[1])); }
        else asm volatile("v_accvgpr_write_b32 a[%2], %0\n\tv_accvgpr_write_b32 a[%3], %1" ::"v"(t[0]), "v"(t[1]), "n"(R), "n"(R + 1));
    }
}
template <bool F16, bool RELU, int R>
__device__ __forceinline__ void pack_whole(const f32x4& acc) {
    unsigned t[2];
    pack_stage<F16, RELU, R, 0>(acc, t); pack_stage<F16, RELU, R, 1>(acc, t); pack_stage<F16, RELU, R, 2>(acc, t);
}
// register of the fragment file that receives tile T of a layer written into set SET, for point tile P
__host__ __device__ constexpr int tile_reg(int np, int set, int p, int t) { return frag_reg(np, set, p, t >> 1) + 2 * (t & 1); }

// The standard schedule of a job's packing work (jobs of >= 8 k-steps).  The gap behind MFMA 0 of a group carries the ring
// bookkeeping, so packing rides in the other gaps.
//   NP = 4: the previous job's point tile pp is packed in group pp + 1, stages 0 / 1 / 2 in the gaps behind MFMAs 1 / 2 / 3.
//           Done by group 4.
//   NP = 2: one gap per group: tile 0 in groups 1, 2, 3, tile 1 in groups 3, 4, 5 (group 3 carries two stages).  Done by group 5.
// Either way the half fragment packed across a layer boundary (it feeds k-step 7) is written >= 2 MFMA issues before its reader,
// and a tile's first stage is >= 5 MFMA issues (80 cycles) behind the MFMA that finished it.
template <bool F16, int NP, bool RELU, int SET, int T, int KS, int P>
__device__ __forceinline__ void pack_sched(const f32x4 (&prev)[NP], unsigned (&t)[NP][2]) {
    if constexpr (NP == 4) {
        if constexpr (KS >= 1 && KS <= NP && P >= 1) pack_stage<F16, RELU, tile_reg(NP, SET, KS - 1, T), P - 1>(prev[KS - 1], t[KS - 1]);
    } else {
        static_assert(NP == 2, "packing schedules exist for 4 and 2 point tiles per wave");
        if constexpr (P == 1 && KS >= 1 && KS <= 3) pack_stage<F16, RELU, tile_reg(NP, SET, 0, T), KS - 1>(prev[0], t[0]);
        if constexpr (P == 1 && KS >= 3 && KS <= 5) pack_stage<F16, RELU, tile_reg(NP, SET, 1, T), KS - 3>(prev[1], t[1]);
    }
}

// ---------------------------------------------------------------------------------------------
// One job: output tile of 16 features x NP point tiles over KS k-steps, stream quads Q0..Q0+KS-1 of the current body
// (bodies start on a slot boundary, so every ring position below is a compile-time constant).
// csel(p): C operand of point tile p's first MFMA (the bias).  bsrc(p_c, ks_c): B operand -- IC<register> (fragment file) or a
// VGPR fragment.  Group ks = NP sub-groups [MFMA of point tile p on fragment a[(Q0+ks) % DA]] [p == 0: ring bookkeeping -- advance,
// one DMA, the A-pipeline refill of the register the PREVIOUS group consumed] [hook(ks_c, p_c)], each pinned: in-order issue lets
// only ~two VALU instructions ride behind a 16-cycle MFMA before the wave blocks on the next one.
// QEND/QPAD: stream positions >= QEND skip QPAD quads (the padding at the end of the tail body).
// ---------------------------------------------------------------------------------------------
template <bool F16, int NP, int NWV, int Q0, int KS, int QEND, int QPAD, typename CSel, typename BSrc, typename Hook>
__device__ __forceinline__ void job(f32x4 (&acc)[NP], CSel csel, BSrc bsrc, u32x4b (&a)[DA], const char* smem, HRing& ring, int lane, Hook hook) {
    static_for<0, KS>([&](auto ks_c) __attribute__((always_inline)) {
        constexpr int ks = decltype(ks_c)::value;
        constexpr int q0 = Q0 + ks + DA - 1;                              // stream position being read into register q0 % DA
        constexpr int qn = (q0 >= QEND) ? q0 + QPAD : q0;
        static_for<0, NP>([&](auto p_c) __attribute__((always_inline)) {
            constexpr int p = decltype(p_c)::value;
            if constexpr (ks == 0) mfma_first<F16>(acc[p], a[(Q0 + ks) % DA], bsrc(p_c, ks_c), csel(p));
            else mfma_acc<F16>(acc[p], a[(Q0 + ks) % DA], bsrc(p_c, ks_c));
            if constexpr (p == 0) {
                if constexpr (qn % HSLOT_QUADS == 0) hring_advance<NWV, F16>(ring);
                a[q0 % DA] = hring_read<NWV, F16>(smem, ring, lane, qn % HSLOT_QUADS);
            }
            hook(ks_c, p_c);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        });
        // the C operands are dead for the compiler once the first MFMAs are issued, but the matrix pipe reads C for up to 7 wait states
        // after the issue of an 8-pass MFMA (ISA guide 4.5: XDL read srcC -> VALU write): keep their registers out of the allocator's
        // hands until the END OF GROUP 1 -- >= 2 MFMA issues = 8 wait states behind the last MFMA of group 0.  (Until round 4 this
        // sat behind group 0, zero wait states after its last MFMA: at the 32-point shape hipcc put the ring's `v_add_u32 fetch_off`
        // into the bias register right there -- tools/mfma_hazard_check.py; no wrong result was ever observed.)
        static_assert(KS >= 2, "a job has at least two k-steps");
        if constexpr (ks == 1) {
            asm volatile("" ::"v"(csel(0)), "v"(csel(1)));
            if constexpr (NP == 4) asm volatile("" ::"v"(csel(2)), "v"(csel(3)));
        }
    });
}

// One PHASE of a launch: ph.n_iter units of NP point tiles per wave over the tiles [ph.tile0, ph.tile_end).  A launch is one phase
// (one shape) or two (whole rounds of the 64-point shape, then the remainder as one round of the 32-point shape): the weight
// ring and the A-fragment pipeline run on across the phase boundary (every unit ends at stream position 0).
template <int W, int LX, int LD, int NP, int NWV, bool F16>
__device__ __forceinline__ void run_phase(const MlpArgsB& a, const PhaseB ph, char* smem, float* side, float* scr_base, char* pe_base, HRing& ring,
                                          u32x4b (&aq)[DA], const int lane, const int wave
#ifdef MN_DIAG
                                          , unsigned long long (&seg)[8], unsigned long long& tprev
#endif
                                          ) {
    constexpr int NT = W / MT, KH = W / KF, KPE = enc_ksteps32(LX);
    constexpr int NTL = NP / 2;                              // 32-sample tiles per unit of work (point tile p: tile p >> 1, half p & 1)
    static_assert(KPE == 2 && NT == 16 && KH == 8 && (NP == 4 || NP == 2), "stream positions and the fragment file are laid out for 63 -> 64 encoded channels, W = 256, 4 or 2 point tiles");
    constexpr int BIG = 1 << 30;
    const int col = lane & 15, q4 = lane >> 4;               // point of a 16-point tile; lane quarter
    const int pq = q4 & (NP - 1);                            // the point tile whose point `col` this lane encodes (NP = 2: quarters 2, 3 duplicate 0, 1)
    float* scratch = scr_base + wave * (NTL * (W / 2));      // per wave, per 32-sample tile: hoisted direction bias
    char* pe_wave = pe_base + wave * (NP * KPE * QUAD_BYTES);    // this wave's parked gamma(x) fragments
    char* pe_lds = pe_wave + lane * 16;
    // ---- tile walk: a wave takes UNITS of NTL consecutive 32-sample tiles = NP 16-point MFMA tiles (point tile p: 32-sample tile
    // p >> 1, half p & 1; a pair of tiles at NP = 4, one tile at NP = 2).  Ray-major (ppr > 0): a wave walks whole rays, so the
    // hoisted view-direction term is computed once per ray; flat otherwise (walk_plan.h).  Inputs of the next unit are loaded a unit ahead.
    const unsigned NW = gridDim.x * NWV, wid = blockIdx.x * NWV + wave;
    // gamma(x) is computed ONCE per point: lane (q4, col) owns point `col` of point tile q4 (32-sample tile q4 >> 1, half q4 & 1),
    // encodes it and writes its fragments' dwords where the other lane quarters read them (the fragments are parked in LDS for the
    // skip layer anyway).  Each lane therefore loads one depth; the rays of both 32-sample tiles are loaded by every lane (the
    // hoisted view-direction term is computed per tile by the whole wave).
    unsigned n_tile[NTL];  float nx_r[NTL][6], nx_z;
    auto load_inputs = [&](unsigned it) __attribute__((always_inline)) {
        const unsigned pr = walk_unit(it, ph.ppr, NW, wid);
        unsigned my_ray = 0, my_chunk = 0;                        // the tile this lane's own point belongs to (selected, not branched on: a lane-
#pragma unroll
        for (int tl = 0; tl < NTL; ++tl) {                        // dependent branch inside the MFMA stream costs a lone wave more than the select)
            unsigned t = ph.tile0 + (unsigned)NTL * pr + tl;
            n_tile[tl] = t;
            if (t >= ph.tile_end) t = ph.tile_end - 1;            // inactive: recompute the last tile, store nothing
            const unsigned ray = t / (unsigned)a.tpr, chunk = t - ray * (unsigned)a.tpr;
            const float* rp = a.rays + (size_t)ray * 6;
#pragma unroll
            for (int e = 0; e < 6; ++e) nx_r[tl][e] = rp[e];
            if (tl == 0 || tl == (pq >> 1)) { my_ray = ray; my_chunk = chunk; }
        }
        {
            const int sample = (int)my_chunk * 32 + 16 * (pq & 1) + col;
            const int sc = sample < a.S ? sample : a.S - 1;
            if (a.z) nx_z = a.z[(size_t)my_ray * a.S + sc];
            else {              // the coarse pass of render_rays: stratified depth drawn here (nerf_process.py:42-60), kept for the compositing
                nx_z = stratified_depth((long long)my_ray, sc, a.S, a.strat_step, a.strat_near, a.strat_far, a.strat_jitter);
                if (q4 < NP) a.z_out[(size_t)my_ray * a.S + sc] = nx_z;      // inactive / clamped lanes rewrite an existing element with its own value
            }
        }
    };
    load_inputs(0);
    unsigned bias_ray[NTL];
#pragma unroll
    for (int tl = 0; tl < NTL; ++tl) bias_ray[tl] = ~0u;

    f32x4 acc[NP], prev[NP];
    f32x4 cin, cnext;                                        // bias of the current / next job (shared by the point tiles)
    auto csel1 = [&](int) __attribute__((always_inline)) -> const f32x4& { return cin; };
    u32x4b peb[NP][KPE];

    // ---- bodies (straight-line code, everything static) ------------------------------------------------------------------------
    // A trunk layer reads fragment set SIN (the second half of fragment 7 is still being packed from `prev` when it starts),
    // writes set 1 - SIN, leaves its last tile in `prev`; the bias of the NEXT job is read while a job's last groups compute.
    auto trunk_layer = [&](auto skip_c, auto sin_c, const float* bias, const float* next_bias) __attribute__((always_inline)) {
        constexpr bool SKIP = decltype(skip_c)::value;
        constexpr int SIN = decltype(sin_c)::value, SOUT = 1 - SIN;
        constexpr int KS = SKIP ? KH + KPE : KH;
        // skip layer: the gamma(x) fragments were parked in LDS by the prologue (32 registers that would otherwise stay live
        // through every layer); each job re-reads them just in time, under its own activation k-steps
        u32x4b per[NP][KPE];
        auto bsrc = [&](auto p_c, auto ks_c) __attribute__((always_inline)) -> decltype(auto) {
            constexpr int p = decltype(p_c)::value, ks = decltype(ks_c)::value;
            if constexpr (ks >= KH) return (const u32x4b&)per[p][ks - KH];
            else return IC<frag_reg(NP, SIN, p, ks)>{};
        };
        static_for<0, NT>([&](auto t_c) __attribute__((always_inline)) {
            constexpr int t = decltype(t_c)::value;
            unsigned pt[NP][2];
            auto hook = [&](auto ks_c, auto p_c) __attribute__((always_inline)) {
                constexpr int ks = decltype(ks_c)::value, p = decltype(p_c)::value;
                // previous tile -> (half a) fragment of the layer that follows it
                if constexpr (t == 0) pack_sched<F16, NP, true, SIN, NT - 1, ks, p>(prev, pt);
                else pack_sched<F16, NP, true, SOUT, t - 1, ks, p>(prev, pt);
                if constexpr (ks == 5 && p == 1) {              // bias of the next job (C operand of its first MFMAs)
                    const float* v = (t + 1 < NT) ? bias + MT * (t + 1) + 4 * q4 : next_bias + 4 * q4;
                    cnext = *(const f32x4*)v;
                }
                if constexpr (SKIP && ks >= KH - 2 && ks < KH - 2 + KPE)         // gamma(x) fragment of k-step ks + 2, one point tile per gap
                    per[p][ks - (KH - 2)] = *(const u32x4b*)(pe_lds + (p * KPE + (ks - (KH - 2))) * QUAD_BYTES);
            };
            job<F16, NP, NWV, t * KS, KS, BIG, 0>(acc, csel1, bsrc, aq, smem, ring, lane, hook);
#pragma unroll
            for (int p = 0; p < NP; ++p) prev[p] = acc[p];
            cin = cnext;
        });
    };

    for (unsigned it = 0; it < ph.n_iter; ++it) {
        // ---- prologue: this pair's points, gamma(x) fragments, hoisted view-direction bias ------------------------------------
        unsigned tray[NTL]; bool valid[NP]; size_t out_idx[NP];
        float in_o[NTL][3], in_d[NTL][3];
        const float in_z = nx_z;
#pragma unroll
        for (int tl = 0; tl < NTL; ++tl) {
            const bool active = n_tile[tl] < ph.tile_end;
            const unsigned t = active ? n_tile[tl] : ph.tile_end - 1;
            const unsigned ray = t / (unsigned)a.tpr, chunk = t - ray * (unsigned)a.tpr;
            tray[tl] = ray;
#pragma unroll
            for (int h = 0; h < 2; ++h) {                       // results of point tile p = 2 tl + h land on lane quarter 0, lane = point
                const int sample = (int)chunk * 32 + 16 * h + col;
                valid[2 * tl + h] = active && sample < a.S;
                out_idx[2 * tl + h] = (size_t)ray * a.S + (sample < a.S ? sample : a.S - 1);
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) { in_o[tl][e] = nx_r[tl][e]; in_d[tl][e] = nx_r[tl][3 + e]; }
        }
        {
            const bool t1 = (pq >> 1) != 0;                     // this lane's point belongs to the second 32-sample tile (NP = 4 only)
            auto mine = [&](const float (&v)[NTL][3], int c) __attribute__((always_inline)) -> float {
                if constexpr (NTL == 2) return t1 ? v[1][c] : v[0][c];
                else return v[0][c];
            };
            const float my_o[3] = {mine(in_o, 0), mine(in_o, 1), mine(in_o, 2)}, my_d[3] = {mine(in_d, 0), mine(in_d, 1), mine(in_d, 2)};
            float pt[3];
            sample_point(pt, my_o, my_d, in_z);
            float sn[LX][3], cs[LX][3];
            // f16: every channel evaluated on its own, as the split-precision kernel does (mlp_f16.hip: why not angle doubling)
            if constexpr (F16) sincos_octaves<LX>(pt, point_is_fast<LX>(pt), sn, cs);
            else
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // octave 0: Cody-Waite + Cephes as in the fp32 kernel, with no libm path.  The multiple count rint(y * 2/pi) is an fp32
                // product: from about 2^20 rad on it is off by one often enough that |r| leaves the polynomials' interval (common.h),
                // and beyond 2^22 it is no longer an integer count at all (an fp32 argument with ulp >= 0.25 rad has no meaningful sine
                // anyway): the remainder is clamped so that finite inputs give finite, bounded encodings (|gamma| <= 1.1 after nine
                // doublings, tests/test_gpu_far_points.py); NaN / Inf still come out as NaN.  (The fp32 kernel takes the libm path there.)
                float r, sp, cp; int q;
                sc_reduce(pt[c], 0, r, q);
                r = __builtin_fminf(__builtin_fmaxf(r, -0.8f), 0.8f) + (r - r);      // (r - r): 0, or NaN for a non-finite remainder
                sc_poly(r, sp, cp);
                sn[0][c] = sc_select(sp, cp, q);
                cs[0][c] = sc_select(sp, cp, q + 1);
#pragma unroll
                for (int k = 1; k < LX; ++k) {                  // angle doubling
                    const float s2 = sn[k - 1][c] + sn[k - 1][c];
                    sn[k][c] = s2 * cs[k - 1][c];
                    cs[k][c] = __builtin_fmaf(-s2, sn[k - 1][c], 1.0f);
                }
            }
            auto chan = [&](int u) __attribute__((always_inline)) -> float { return gamma_channel<LX>(u, pt, sn, cs); };
            // fragment (point tile pq, k-step ks): lane quarter qq reads channels 32 ks + 8 qq + j of point `col` at
            // [fragment][(qq * 16 + col) * 16 bytes]: this lane writes those 16 bytes for every qq (at NP = 2 lane quarters 2, 3
            // write what quarters 0, 1 write: same bytes, same addresses)
            char* wr = pe_wave + (pq * KPE) * QUAD_BYTES + col * 16;
#pragma unroll
            for (int ks = 0; ks < KPE; ++ks)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) {
                    u32x4b v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = pack2<F16>(chan(KF * ks + 8 * qq + 2 * i), chan(KF * ks + 8 * qq + 2 * i + 1));
                    *(u32x4b*)(wr + ks * QUAD_BYTES + qq * 256) = v;
                }
        }
        // LDS operations of one wave execute in order: the fragments written above are complete when these reads return
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int ks = 0; ks < KPE; ++ks) peb[p][ks] = *(const u32x4b*)(pe_lds + (p * KPE + ks) * QUAD_BYTES);
        // hoisted view-direction term of linear_d (fp32), per 32-sample tile: scratch[tl][n] = b_d[n] + sum_f Wd[n][W+f] * gamma(d/|d|)[f]
#pragma unroll
        for (int tl = 0; tl < NTL; ++tl) {
            float* sc_t = scratch + tl * (W / 2);
            if (tray[tl] != bias_ray[tl]) {
                bias_ray[tl] = tray[tl];
                if (tl == 1 && tray[NTL - 1] == tray[0]) {      // both tiles on one ray: copy (same wave: no barrier needed)
#pragma unroll
                    for (int n0 = 0; n0 < W / 2; n0 += 64) sc_t[n0 + lane] = scratch[n0 + lane];
                } else {
                    hoisted_dir_bias<W, LD>(sc_t, in_d[tl][0], in_d[tl][1], in_d[tl][2], side + a.o_wdir_t, side + a.o_bias_d, lane);
                }
            }
        }
        BSTAMP(0);   // prologue
        // ---- layer 0: 16 jobs of 2 k-steps over gamma(x) (VGPR fragments), output into set 0 -----------------------------------------
        {
            const float* b0 = side + a.o_bias_trunk + 4 * q4;
            cin = *(const f32x4*)b0;
            auto bsrc = [&](auto p_c, auto ks_c) __attribute__((always_inline)) -> const u32x4b& { return peb[decltype(p_c)::value][decltype(ks_c)::value]; };
            static_for<0, NT>([&](auto t_c) __attribute__((always_inline)) {
                constexpr int t = decltype(t_c)::value;
                auto hook = [&](auto ks_c, auto p_c) __attribute__((always_inline)) {
                    constexpr int ks = decltype(ks_c)::value, p = decltype(p_c)::value;
                    // 2 NP MFMAs per job and NP tiles to pack: a whole statement per gap (these jobs run VALU bound; 3 % of the MFMAs).
                    // A tile is packed >= 4 MFMA issues behind the MFMA that finished it.
                    if constexpr (NP == 4) {
                        if constexpr (t > 0 && ks == 0 && p >= 1) pack_whole<F16, true, tile_reg(NP, 0, p - 1, t - 1)>(prev[p - 1]);
                        if constexpr (t > 0 && ks == 1 && p == 1) pack_whole<F16, true, tile_reg(NP, 0, 3, t - 1)>(prev[3]);
                    } else {
                        if constexpr (t > 0 && ks == 1) pack_whole<F16, true, tile_reg(NP, 0, p, t - 1)>(prev[p]);
                    }
                    if constexpr ((NP == 4 && ks == 1 && p == 2) || (NP == 2 && ks == 0 && p == 1)) {
                        const float* v = (t + 1 < NT) ? b0 + MT * (t + 1) : side + a.o_bias_trunk + W + 4 * q4;
                        cnext = *(const f32x4*)v;
                    }
                };
                job<F16, NP, NWV, t * KPE, KPE, BIG, 0>(acc, csel1, bsrc, aq, smem, ring, lane, hook);
#pragma unroll
                for (int p = 0; p < NP; ++p) prev[p] = acc[p];
                cin = cnext;
            });
        }
        BSTAMP(1);   // layer 0
        // ---- trunk layers 1..D-1 ping-pong between the two fragment sets with a static polarity (pairs 0->1, 1->0) --------------------
        auto layer_01 = [&](int l) __attribute__((always_inline)) {
            const float* bias = side + a.o_bias_trunk + l * W;
            const float* nb = (l + 1 < a.D) ? bias + W : side + a.o_bias_feat;
            if (l == a.skip_layer) trunk_layer(std::true_type{}, IC<0>{}, bias, nb);
            else trunk_layer(std::false_type{}, IC<0>{}, bias, nb);
        };
        auto layer_10 = [&](int l) __attribute__((always_inline)) {
            const float* bias = side + a.o_bias_trunk + l * W;
            const float* nb = (l + 1 < a.D) ? bias + W : side + a.o_bias_feat;
            if (l == a.skip_layer) trunk_layer(std::true_type{}, IC<1>{}, bias, nb);
            else trunk_layer(std::false_type{}, IC<1>{}, bias, nb);
        };
        int l = 1;                                               // layer 0 wrote set 0 (its last tile is still in `prev`)
#pragma unroll 1
        for (; l + 1 < a.D; l += 2) { layer_01(l); layer_10(l + 1); }
        // ---- tail: feature layer, density tile, view-direction layer, colour tile, store ---------------------------------------------
        auto tail = [&](auto sin_c) __attribute__((always_inline)) {
            constexpr int SIN = decltype(sin_c)::value, SOUT = 1 - SIN;
            f32x4 hd[NP], hc[NP], cind[NP], cnextd[NP], cinh;            // density / colour tiles; per-point-tile direction bias
            float dens[NP];
            auto cseld = [&](int p) __attribute__((always_inline)) -> const f32x4& { return cind[p]; };
            auto cselh = [&](int) __attribute__((always_inline)) -> const f32x4& { return cinh; };
            const float* bf = side + a.o_bias_feat + 4 * q4;
            auto bsrc_in = [&](auto p_c, auto ks_c) __attribute__((always_inline)) { return IC<frag_reg(NP, SIN, decltype(p_c)::value, decltype(ks_c)::value)>{}; };
            auto bsrc_out = [&](auto p_c, auto ks_c) __attribute__((always_inline)) { return IC<frag_reg(NP, SOUT, decltype(p_c)::value, decltype(ks_c)::value)>{}; };
            // feature layer: no activation on its outputs; its first job still packs the trunk's last tile (ReLU)
            static_for<0, NT>([&](auto t_c) __attribute__((always_inline)) {
                constexpr int t = decltype(t_c)::value;
                unsigned pt[NP][2];
                auto hook = [&](auto ks_c, auto p_c) __attribute__((always_inline)) {
                    constexpr int ks = decltype(ks_c)::value, p = decltype(p_c)::value;
                    if constexpr (t == 0) pack_sched<F16, NP, true, SIN, NT - 1, ks, p>(prev, pt);
                    else pack_sched<F16, NP, false, SOUT, t - 1, ks, p>(prev, pt);
                    if constexpr (ks == 5 && p == 1) {
                        if constexpr (t + 1 < NT) cnext = *(const f32x4*)(bf + MT * (t + 1));
                        else {                                          // density tile: row 3 = density bias (lane quarter 0 only)
                            const float db = side[a.o_head_b + 3];
                            cnext[0] = 0.0f; cnext[1] = 0.0f; cnext[2] = 0.0f; cnext[3] = q4 == 0 ? db : 0.0f;
                        }
                    }
                };
                job<F16, NP, NWV, t * KH, KH, BIG, 0>(acc, csel1, bsrc_in, aq, smem, ring, lane, hook);
#pragma unroll
                for (int p = 0; p < NP; ++p) prev[p] = acc[p];
                cin = cnext;
            });
            // density tile over the trunk output (row 3); packs the feature layer's last tile; reads the direction bias of tile 0
            {
                unsigned pt[NP][2];
                auto hook = [&](auto ks_c, auto p_c) __attribute__((always_inline)) {
                    constexpr int ks = decltype(ks_c)::value, p = decltype(p_c)::value;
                    pack_sched<F16, NP, false, SOUT, NT - 1, ks, p>(prev, pt);
                    if constexpr (ks == 5) cnextd[p] = *(const f32x4*)(scratch + (p >> 1) * (W / 2) + 4 * q4);
                };
                job<F16, NP, NWV, 128, KH, BIG, 0>(hd, csel1, bsrc_in, aq, smem, ring, lane, hook);
#pragma unroll
                for (int p = 0; p < NP; ++p) cind[p] = cnextd[p];
            }
            // view-direction layer: 8 jobs over the feature layer's output; ReLU'd tiles go into fragments 0..3 of set SIN (the
            // trunk output is dead once the density tile has run)
            static_for<0, NT / 2>([&](auto t_c) __attribute__((always_inline)) {
                constexpr int t = decltype(t_c)::value;
                unsigned pt[NP][2];
                auto hook = [&](auto ks_c, auto p_c) __attribute__((always_inline)) {
                    constexpr int ks = decltype(ks_c)::value, p = decltype(p_c)::value;
                    if constexpr (t > 0) pack_sched<F16, NP, true, SIN, t - 1, ks, p>(prev, pt);
                    if constexpr (t == 0 && ks == 1 && p == NP - 1) {      // the density tile's last MFMA is >= 4 issues back: its tuples may go (keep_tuple, common.h)
#pragma unroll
                        for (int pp = 0; pp < NP; ++pp) keep_tuple(hd[pp]);
                    }
                    if constexpr (t == 0 && ks == 6)            // the density tile finished >= 24 MFMAs ago: keep its one useful register
                        asm volatile("v_mov_b32 %0, %1" : "=v"(dens[p]) : "v"(hd[p][3]));
                    // next pair's rays and depths, two quads BEHIND a ring advance (tail position 162 = slot 5, quad 2): an advance waits for every
                    // older vector memory operation, and two quads before one (position 158, where this sat) is the worst place for a load.  A/B: 0.2 %;
                    // the loads and their index arithmetic cost the kernel 2 % in all (ablation build without them).
                    if constexpr (t == BF16_PF_T && ks == BF16_PF_KS && p == 1) load_inputs(it + 1 < ph.n_iter ? it + 1 : it);
                    if constexpr (ks == 5) {
                        if constexpr (t + 1 < NT / 2) cnextd[p] = *(const f32x4*)(scratch + (p >> 1) * (W / 2) + MT * (t + 1) + 4 * q4);
                        else if constexpr (p == 1) {                    // colour tile: rows 0..2 = colour bias (lane quarter 0 only)
                            const f32x4 hb4 = *(const f32x4*)(side + a.o_head_b);
                            cinh[0] = q4 == 0 ? hb4[0] : 0.0f; cinh[1] = q4 == 0 ? hb4[1] : 0.0f; cinh[2] = q4 == 0 ? hb4[2] : 0.0f; cinh[3] = 0.0f;
                        }
                    }
                };
                job<F16, NP, NWV, 136 + t * KH, KH, BIG, 0>(acc, cseld, bsrc_out, aq, smem, ring, lane, hook);
#pragma unroll
                for (int p = 0; p < NP; ++p) { prev[p] = acc[p]; cind[p] = cnextd[p]; }
            });
            // colour tile over the view-direction output (rows 0..2): 4 k-steps; the last direction tile (second half of fragment 3) is
            // packed in its first groups, a whole statement per gap
            {
                auto hook = [&](auto ks_c, auto p_c) __attribute__((always_inline)) {
                    constexpr int ks = decltype(ks_c)::value, p = decltype(p_c)::value;
                    if constexpr (NP == 4) {
                        if constexpr (ks == 0 && p >= 1) pack_whole<F16, true, tile_reg(NP, SIN, p - 1, NT / 2 - 1)>(prev[p - 1]);
                        if constexpr (ks == 1 && p == 1) pack_whole<F16, true, tile_reg(NP, SIN, 3, NT / 2 - 1)>(prev[3]);
                    } else {                                    // >= 4 MFMA issues behind the tile's last MFMA, two groups ahead of k-step 3
                        if constexpr (ks == 1) pack_whole<F16, true, tile_reg(NP, SIN, p, NT / 2 - 1)>(prev[p]);
                    }
                };
                job<F16, NP, NWV, 200, KH / 2, TAIL_USED, TAIL_QUADS - TAIL_USED>(hc, cselh, bsrc_in, aq, smem, ring, lane, hook);
            }
            // the MFMAs are asm statements: hipcc does not know that `hc` is still in flight (XDL write -> vector-memory read)
            asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
            for (int p = 0; p < NP; ++p) keep_tuple(hc[p]);     // element 3 is never read: whole tuples stay allocated until here
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (valid[p] && q4 == 0) {                      // cat([rgb, density]) NeRF.py:51
                    f32x4 o; o[0] = hc[p][0]; o[1] = hc[p][1]; o[2] = hc[p][2]; o[3] = dens[p];
                    *(f32x4*)(a.out + out_idx[p] * 4) = o;
                }
        };
        if (l < a.D) { layer_01(l); BSTAMP(2); tail(IC<1>{}); }
        else { BSTAMP(2); tail(IC<0>{}); }
        BSTAMP(3);   // tail
    }
}

// NWV waves per workgroup: 4 (one wave per SIMD: the 64-point shape needs the whole register file) or 8 (two waves per SIMD, 32-point
// shape only: 120 VGPRs + the 128 AGPRs of its fragment file fit twice; the partner wave's MFMAs fill the issue slots a wave loses
// to its DMA issues, packing and LDS waits, at the 64-point shape's 256 points per pass of the weight stream).
// The kernel body; mlp_bf16_kernel / mlp_f16_kernel below are its two element types (one per translation unit).
template <int W, int LX, int LD, int NPA, int NPB, int NWV, bool F16>
__device__ __forceinline__ void mlp_half_body(const MlpArgsB& a) {
    static_assert(W == 256, "bf16 / f16 variant: W = 256");
    static_assert(NWV == 4 || (NWV == 8 && NPA == 2 && NPB == 0), "two waves per SIMD: the 32-point shape only");
    constexpr int NPM = NPA > NPB ? NPA : NPB;
    // reserve the fragment file (see THE FRAGMENT FILE): the whole accumulation-register file, or its lower half
    if constexpr (NWV == 4) asm volatile("" ::: "a255");
    else asm volatile("" ::: "a127");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* side = (float*)(smem + HRING_BYTES);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (unsigned i = tid * 4; i < a.side_floats; i += 64 * NWV * 4) *(f32x4*)(side + i) = *(const f32x4*)(a.side + i);
    float* scr_base = side + a.side_floats;
    char* pe_base = (char*)(scr_base + NWV * (NPM / 2) * (W / 2));

    HRing ring = hring_start<NWV, F16>(a.stream, a.stream_bytes, smem, wave, lane);
#pragma unroll
    for (int i = 0; i < hring_dmas(NWV); ++i) hring_dma<NWV, F16>(ring, i);       // slot 0
    hring_next_fetch<F16>(ring);
#pragma unroll
    for (int i = 0; i < hring_dmas(NWV); ++i) hring_dma<NWV, F16>(ring, i);       // slot 1; slot p+2 streams in while slot p is consumed

    u32x4b aq[DA];
    hring_advance<NWV, F16>(ring);                           // also publishes the side tables (barrier)
#pragma unroll
    for (int i = 0; i < DA - 1; ++i) aq[i] = hring_read<NWV, F16>(smem, ring, lane, i);      // position q is read while group q - (DA - 1) computes

#ifdef MN_DIAG
    unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev = bstamp();
    run_phase<W, LX, LD, NPA, NWV, F16>(a, a.ph[0], smem, side, scr_base, pe_base, ring, aq, lane, wave, seg, tprev);
    if constexpr (NPB != 0) run_phase<W, LX, LD, NPB, NWV, F16>(a, a.ph[1], smem, side, scr_base, pe_base, ring, aq, lane, wave, seg, tprev);
#else
    run_phase<W, LX, LD, NPA, NWV, F16>(a, a.ph[0], smem, side, scr_base, pe_base, ring, aq, lane, wave);
    if constexpr (NPB != 0) run_phase<W, LX, LD, NPB, NWV, F16>(a, a.ph[1], smem, side, scr_base, pe_base, ring, aq, lane, wave);
#endif
#ifdef MN_DIAG
    if (a.diag && lane == 0) {
        unsigned long long* d = a.diag + ((size_t)blockIdx.x * NWV + wave) * 8;
        for (int i = 0; i < 8; ++i) d[i] = seg[i];
    }
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- small coarse launch: render_rays' middle for the two rays this workgroup owns (nerf_process.py:198-203) -----------------------------
    // One 32-point unit per wave, flat walk, 64 samples = two units per ray: waves 4b .. 4b + 3 computed rays 2b and 2b + 1 whole.  Their raw
    // outputs and depths are in global memory (the stores above have completed: vmcnt(0); same CU, same L1: nothing to invalidate at workgroup
    // scope), the weight ring is quiescent (its last DMAs have landed) and becomes the two waves' scratch.  Waves 0 and 1 each run the SAME
    // device functions the stage kernel runs (composite_fine_z_kernel, stages.hip): identical results, one launch and ~4 us fewer per step
    // at the 512-ray shard of an 8-GPU split.  Larger launches leave it to the stage kernel (a wave per ray there, thousands in flight).
    if constexpr (NPA == 2 && NPB == 0 && NWV == 4) {
        if (a.fz_on) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            const long long ray = 2ll * blockIdx.x + wave;
            if (wave < 2 && ray < (long long)a.n_rays) {
                float* mine = (float*)smem + wave * (a.S + 2 * (a.S - 1) + a.fz_n2);
                composite_ray<1>(a.out, a.z_out, a.rays, 6, ray, a.S, lane, a.fz_rgb, a.fz_disp, nullptr, a.fz_w, nullptr, mine);
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                fine_z_ray(a.z_out, mine, ray, a.S, a.fz_Nf, a.fz_n2, a.fz_det, a.fz_u, a.fz_zf, nullptr, mine + a.S, lane);
            }
        }
    }
    // The same one step up in size (513..1024 rays on 256 CUs): one 64-point unit per wave and 33..64 coarse samples = one unit per RAY, so every wave
    // owns the ray it computed and does the middle for it (all four waves busy; each its own slice of the quiescent ring).
    if constexpr (NPA == 4 && NPB == 0 && NWV == 4) {
        if (a.fz_on) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            const long long ray = 4ll * blockIdx.x + wave;
            if (ray < (long long)a.n_rays) {
                float* mine = (float*)smem + wave * (a.S + 2 * (a.S - 1) + a.fz_n2);
                composite_ray<1>(a.out, a.z_out, a.rays, 6, ray, a.S, lane, a.fz_rgb, a.fz_disp, nullptr, a.fz_w, nullptr, mine);
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                fine_z_ray(a.z_out, mine, ray, a.S, a.fz_Nf, a.fz_n2, a.fz_det, a.fz_u, a.fz_zf, nullptr, mine + a.S, lane);
            }
        }
    }
}

template <int W, int LX, int LD, int NPA, int NPB, int NWV>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(NWV / 4, NWV / 4)))
void mlp_bf16_kernel(const MlpArgsB a) { mlp_half_body<W, LX, LD, NPA, NPB, NWV, false>(a); }
template <int W, int LX, int LD, int NPA, int NPB, int NWV>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(NWV / 4, NWV / 4)))
void mlp_f16_kernel(const MlpArgsB a) { mlp_half_body<W, LX, LD, NPA, NPB, NWV, true>(a); }

// The walk of one phase: shape NP over the tiles [tile0, tile_end) on a grid of `grid` workgroups.
template <int NP, int NWV>
static PhaseB make_phase(const MlpArgsB& a, long long tile0, long long tile_end, int grid) {
    constexpr int NTL = NP / 2;
    PhaseB ph{};
    ph.tile0 = (unsigned)tile0; ph.tile_end = (unsigned)tile_end;
    const long long n_units = (tile_end - tile0 + NTL - 1) / NTL;
    const long long n_rays = (tile_end + a.tpr - 1) / a.tpr;     // rays this phase touches when it starts at tile 0
    // whole rays per wave (tiles >= tile_end are skipped) only for a phase that starts at a ray's first tile, with rays of whole units
    const WalkPlan plan = walk_plan(n_rays, a.tpr / NTL, n_units, grid, NWV, tile0 == 0 && a.tpr % NTL == 0);
    ph.ppr = plan.ray_major ? (unsigned)(a.tpr / NTL) : 0;
    ph.n_iter = (unsigned)plan.n_iter;
    return ph;
}

// One launch: phase A of shape NPA over [0, split), then (NPB != 0) phase B of shape NPB over [split, n_wtiles).
template <int NPA, int NPB, int NWV, bool F16>
static int launch_half(MlpArgsB a, long long split, long long n_wtiles, hipStream_t st) {
    constexpr int NPM = NPA > NPB ? NPA : NPB;
    // ring | side tables | per wave: a hoisted direction bias [W/2] per 32-point tile, the parked gamma(x) fragments [NPM][KPE] quads
    constexpr auto lds_bytes = [](int D) { return (size_t)HRING_BYTES + half_side_bytes(D) + (size_t)NWV * (NPM / 2) * (256 / 2) * 4 + (size_t)NWV * NPM * enc_ksteps32(10) * QUAD_BYTES; };
    static_assert(NPM == 4 ? (lds_bytes(HALF_64PT_MAX_D) <= LDS_BYTES && lds_bytes(HALF_64PT_MAX_D + 1) > LDS_BYTES) : lds_bytes(16) <= LDS_BYTES,
                  "the 64-point shape holds HALF_64PT_MAX_D layers' tables, the 32-point shape every depth check_net_half accepts");
    MN_CHECK_ARG(NPM != 4 || a.D <= HALF_64PT_MAX_D, "the 64-points-per-wave shape of the %s kernel keeps every layer's biases and 36 KiB of per-wave buffers beside the weight ring "
                 "in LDS: D = %d does not fit (D <= %d); points_per_wave 0 or 32 runs a deeper network at 32 points per wave", F16 ? "f16" : "bf16", a.D, HALF_64PT_MAX_D);
    const size_t lds = lds_bytes(a.D);
    MN_CHECK_ARG((size_t)a.side_floats * 4 == half_side_bytes(a.D) && lds <= LDS_BYTES, "internal: this launch of a %d-deep network needs %zu bytes of LDS", a.D, lds);
    auto kern = [] {                                         // only the element type of this translation unit is instantiated
        if constexpr (F16) return mlp_f16_kernel<256, 10, 4, NPA, NPB, NWV>;
        else return mlp_bf16_kernel<256, 10, 4, NPA, NPB, NWV>;
    }();
    static LdsOptIn opt_in = {};
    if (int rc = ensure_lds_opt_in(opt_in, (const void*)kern)) return rc;
    const long long wg_a = ((split + NPA / 2 - 1) / (NPA / 2) + NWV - 1) / NWV;
    constexpr int TPB = NPB ? NPB / 2 : 1;                    // tiles per unit of the second phase (1: no second phase, wg_b unused)
    const long long wg_b = NPB ? ((n_wtiles - split + TPB - 1) / TPB + NWV - 1) / NWV : 0;
    const int grid = persistent_grid(wg_a > wg_b ? wg_a : wg_b);
    a.ph[0] = make_phase<NPA, NWV>(a, 0, split, grid);
    if constexpr (NPB != 0) a.ph[1] = make_phase<NPB, NWV>(a, split, n_wtiles, grid);
#ifdef MN_DIAG
    {   // diagnostic build: run once with stamps and print the per-segment averages (cycles per unit per wave; single-phase launches)
        unsigned long long* dbuf = nullptr;
        const size_t n = (size_t)grid * NWV * 8;
        MN_HIP(hipMalloc(&dbuf, n * 8));
        MN_HIP(hipMemsetAsync(dbuf, 0, n * 8, st));
        a.diag = dbuf;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NWV), lds, st, a);
        MN_HIP(hipStreamSynchronize(st));
        std::vector<unsigned long long> hbuf(n);
        MN_HIP(hipMemcpy(hbuf.data(), dbuf, n * 8, hipMemcpyDeviceToHost));
        (void)hipFree(dbuf);
        static const char* names[4] = {"prologue", "layer0", "trunk", "tail"};
        const char* tag = F16 ? "f16" : "bf16";
        const double ideal[4] = {0, 512.0 * NPA, (7 * 2048 + 512.0) * NPA, 204 * 16.0 * NPA};
        double tot = 0;
        const unsigned n_iter = a.ph[0].n_iter + (NPB ? a.ph[1].n_iter : 0);
        fprintf(stderr, "[mn_diag %s] NP=%d(+%d) grid=%d units/wave=%u  cycles per unit (mean over waves; ideal MFMA cycles of the first shape in brackets):\n",
                tag, NPA, NPB, grid, n_iter);
        for (int sgi = 0; sgi < 4; ++sgi) {
            double sum = 0;
            for (size_t w = 0; w < (size_t)grid * NWV; ++w) sum += (double)hbuf[w * 8 + sgi];
            const double per = sum / ((double)grid * NWV) / (double)n_iter;
            tot += per;
            fprintf(stderr, "[mn_diag %s]   %-10s %10.0f  [%6.0f]\n", tag, names[sgi], per, ideal[sgi]);
        }
        fprintf(stderr, "[mn_diag %s]   %-10s %10.0f  [%6.0f]\n", tag, "total", tot, ideal[1] + ideal[2] + ideal[3]);
        return MI_NERF_OK;
    }
#endif
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NWV), lds, st, a);
    if constexpr (F16) MN_LAUNCH_CHECK("mlp_f16_kernel");
    else MN_LAUNCH_CHECK("mlp_bf16_kernel");
    return MI_NERF_OK;
}

// The launch plan (mlp_rays_bf16 / mlp_rays_f16; the caller has checked the network).  L: the blob's layout (half_layout.h); the ring
// walks L.walk_bytes of stream (bf16: the blob's stream; f16: body + 224 positions of 2 KiB, see hring_next_fetch).
// points_per_wave: 0 = chosen per launch (pick_np), 64 / 32 = forced (A/B measurements, parity tests of each shape)
// z_dev == NULL (strat != NULL): the kernel draws the stratified depths of render_rays' coarse pass itself and writes them to strat->z_out
template <bool F16>
static int mlp_rays_half(const mi_nerf_net* net, const HalfLayout& L, const void* packed_dev, const float* rays_dev, const float* z_dev, int64_t n_rays,
                         int S, float* raw_dev, hipStream_t st, int points_per_wave, const StratDraw* strat, FineDraw* fine) {
    MN_CHECK_ARG(n_rays >= 0 && S >= 1, "bad sizes n_rays=%lld S=%d", (long long)n_rays, S);
    MN_CHECK_ARG(points_per_wave == 0 || points_per_wave == 32 || points_per_wave == 64, "points_per_wave must be 0 (auto), 32 or 64 (got %d)",
                 points_per_wave);
    if (n_rays == 0) return MI_NERF_OK;
    MN_CHECK_ARG(packed_dev && rays_dev && raw_dev && (z_dev || (strat && strat->z_out)), "NULL device pointer");
    MlpArgsB a{};
    if (!z_dev) {
        a.z_out = strat->z_out; a.strat_near = strat->near_; a.strat_far = strat->far_;
        a.strat_step = S > 1 ? 1.0f / (float)(S - 1) : 0.0f;
        a.strat_jitter = Jitter{strat->t_rand, strat->seed, 0u, (long long)strat->ray0};
    }
    (SideTables&)a = side_tables(L, packed_dev, net->D, net->skip, L.walk_bytes);
    a.rays = rays_dev; a.z = z_dev; a.out = raw_dev;
    a.S = S; a.tpr = (S + 31) / 32;
    const long long n_wtiles = (long long)n_rays * a.tpr;
    MN_CHECK_ARG(n_wtiles < (1LL << 30), "too many points for one launch: %lld rays x %d samples", (long long)n_rays, S);
    a.n_rays = (unsigned)n_rays;
    if (points_per_wave == 64) return launch_half<4, 0, 4, F16>(a, n_wtiles, n_wtiles, st);
    // ... and a network deeper than the 64-point shape's LDS holds (HALF_64PT_MAX_D: half_layout.h) runs every launch at 32 points per wave
    if (points_per_wave == 32 || net->D > HALF_64PT_MAX_D) return launch_half<2, 0, 4, F16>(a, n_wtiles, n_wtiles, st);
    // (An 8-wave shape -- 32 points per wave, two waves per SIMD -- was measured SLOWER than the 64-point shape at every size: 4096 rays, fine
    // launch 638 vs 603 us, profiles/r03_bf16_two_waves_per_simd.txt.  The kernel is not short of latency hiding, it is short of power: twice
    // the LDS reads per FLOP cost more clock than the interleaving wins back.  Its instantiation is gone: tools/ABLATIONS.md.)
    // The launch plan.  A pass of the 64-point shape takes the same time whatever the number of active CUs (the kernel is bound by
    // what ONE CU does per pass), a pass of the 32-point shape ~0.65 of it (half the matrix work, the same weight stream:
    // profiles/r03_bf16_small_launch_shape.txt).  So: whole rounds of the 64-point shape (every wave of the chip a pair of tiles),
    // then the remainder as ONE round of the 32-point shape if it fits one (every wave one tile), else as one more 64-point round;
    // both phases in ONE launch (the weight ring streams on across the phase boundary).
    // A 512-ray shard of BASELINE config #5 (8 GPUs): coarse 1024 tiles = one 32-point round (was half the chip for a full pass);
    // fine 3072 tiles = one 64-point round + one 32-point round (was two full passes, the second half empty).
    const long long round4 = (long long)device_cus() * 4 * 2, round2 = (long long)device_cus() * 4;
    // render_rays' middle in the coarse launch's epilogue (`fine` offered; a coarse pass of 33..64 samples; one unit per wave, flat walk -- which is what
    // the epilogue's ray numbering assumes): `slices` waves of a workgroup each take a ray and a slice of the ring as scratch
    auto take_middle = [&](int slices) {
        if (!(fine && !z_dev && a.tpr == 2 && fine->Nf >= 1 && S >= 3)) return;
        int n2 = 2;
        while (n2 < S + fine->Nf) n2 <<= 1;
        const size_t scratch = (size_t)slices * (S + 2 * (S - 1) + n2) * sizeof(float);
        if (scratch > (size_t)HRING_BYTES || n2 > 512) return;
        a.fz_on = 1; a.fz_Nf = fine->Nf; a.fz_n2 = n2; a.fz_det = fine->det;
        a.fz_u = Jitter{fine->u, fine->seed, 1u, (long long)fine->ray0};
        a.fz_rgb = fine->rgb_c; a.fz_disp = fine->disp_c; a.fz_w = fine->w_c; a.fz_zf = fine->z_f;
        fine->taken = true;
    };
    const long long main_tiles = (n_wtiles / round4) * round4, rem = n_wtiles - main_tiles;
    if (rem == 0 || rem > round2) {
        // at most one 64-point unit per wave and one unit per ray (33..64 samples): every wave owns the ray it computes (513..1024 rays on 256 CUs)
        if (n_wtiles <= round4) take_middle(4);
        return launch_half<4, 0, 4, F16>(a, n_wtiles, n_wtiles, st);
    }
    if (main_tiles == 0) {
        // one round of 32-point units, one unit per wave.  A coarse pass of 33..64 samples is two units per ray, so a workgroup's four waves hold
        // two rays whole: it takes render_rays' middle for them too when the caller offers it (`fine`; the kernel's epilogue).  The grid is one
        // workgroup per four tiles and the walk flat (n_iter == 1: make_phase), which is what the epilogue's ray = 2 * block + wave assumes.
        take_middle(2);
        return launch_half<2, 0, 4, F16>(a, n_wtiles, n_wtiles, st);
    }
    return launch_half<4, 2, 4, F16>(a, main_tiles, n_wtiles, st);
}


}  // namespace minerf
