// half_layout.h -- host side of the 16-bit weight blobs (v_mfma_f32_16x16x32_*): their one stream order and layout, the network check of
// the variants that read them, and the packer entry points (pack_half.hip; pack.cpp for the fp32 blobs).
//
// Three blob kinds share the stream order described in mlp_bf16.hip (output-tile-major jobs of 1 KiB quads, the same tail):
//   kind 3  bf16 forward              one quad per stream position                              mlp_bf16.hip
//   kind 4  split-precision forward   a (hi, lo) PAIR of f16 quads per position (2 KiB)         mlp_f16s.hip; mlp_f16.hip reads the hi quads
//   kind 5  split-precision backward  pairs of the transposed chain, no side tables             dgrad_f16s.hip
#pragma once
#include <vector>
#include "common.h"
#include "layout.h"

namespace minerf {

constexpr int MT = 16;                                     // output features per job
constexpr int KF = 32;                                     // k per MFMA
constexpr int TAIL_USED = 128 + 8 + 64 + 4;                // stream positions of the tail body that carry weights (quads, or pairs)
constexpr int TAIL_QUADS = 224;                            // ... padded to whole ring slots: bf16 (7 slots of 32 quads)
constexpr int TAIL_PAIRS = 208;                            // ... split precision (416 quads = 13 slots)
__host__ __device__ constexpr int enc_ksteps32(int L) { return (3 + 6 * L + KF - 1) / KF; }
constexpr float SPLIT_SCALE = 2048.0f;                     // split precision: x = x_hi + x_lo * 2^-11 (mlp_f16s.hip)

enum class HalfStream { QUADS, PAIRS };                    // what a stream position holds: a bf16 quad, or a (hi, lo) pair of f16 quads

// The forward blob (header | stream | fp32 side tables) as the kernels read it.
struct HalfLayout {
    uint32_t stream_off, stream_bytes, side_off, side_floats;
    uint32_t bias_trunk, bias_feat, bias_d, head_b, wdir_t, total_bytes;      // side-table sub-offsets in floats from side start
    // The stream's length as the ring of mlp_half_core.h walks it: TAIL_QUADS tail positions of this stream's size.  The blob's own stream
    // for QUADS; for PAIRS (the f16 kernel on the split-precision blob) TAIL_QUADS - TAIL_PAIRS positions more than the blob holds -- the
    // last slot re-reads data it never uses instead (hring_next_fetch).
    uint32_t walk_bytes;
};
inline HalfLayout make_half_layout(int D, int W, int skip, HalfStream kind) {
    HalfLayout b{};
    const int NT = W / MT, in_d = 3 + 6 * KERNEL_LD;        // the kernels' encoding; a network with fewer frequencies gets zero weights (layout.h)
    const uint32_t pos_bytes = kind == HalfStream::PAIRS ? 2 * QUAD_BYTES : QUAD_BYTES;
    const uint32_t pe = (uint32_t)enc_ksteps32(KERNEL_LX) * NT, h = (uint32_t)(W / KF) * NT;
    uint32_t body = pe;
    for (int l = 1; l < D; ++l) body += h + ((skip >= 0 && l == skip + 1) ? pe : 0);
    b.stream_off = HEADER_BYTES;
    b.stream_bytes = (body + (kind == HalfStream::PAIRS ? TAIL_PAIRS : TAIL_QUADS)) * pos_bytes;
    b.walk_bytes = (body + TAIL_QUADS) * pos_bytes;
    b.side_off = b.stream_off + b.stream_bytes;
    uint32_t f = 0;
    b.bias_trunk = f; f += (uint32_t)D * W;
    b.bias_feat = f;  f += W;
    b.bias_d = f;     f += W / 2;
    b.head_b = f;     f += 4;                       // colour bias (3), density bias
    b.wdir_t = f;     f += (uint32_t)in_d * (W / 2);
    b.side_floats = round_up_u32(f, 4);
    b.total_bytes = b.side_off + b.side_floats * 4;
    return b;
}
// the record the forward kernels read (layout.h); stream_bytes: L.walk_bytes (mlp_half_core.h's ring) or L.stream_bytes (mlp_f16s_core.h's)
inline SideTables side_tables(const HalfLayout& L, const void* packed_dev, int D, int skip, uint32_t stream_bytes) {
    SideTables t{};
    t.stream = (const char*)packed_dev + L.stream_off;
    t.side = (const float*)((const char*)packed_dev + L.side_off);
    t.D = D;
    t.skip_layer = skip_layer_of(D, skip);
    t.stream_bytes = stream_bytes;
    t.side_floats = L.side_floats;
    t.o_bias_trunk = L.bias_trunk; t.o_bias_feat = L.bias_feat; t.o_bias_d = L.bias_d; t.o_wdir_t = L.wdir_t;
    t.o_head_b = L.head_b;
    return t;
}
// the split-precision backward stream (W = 256): linear_d^T's feature block, linear_feat^T, linear_x[D-1 .. 1]^T, as pairs
inline uint32_t bwd_stream_bytes_s(int D) { return (uint32_t)(16 * 4 + 16 * 8 * D) * 2u * QUAD_BYTES; }

// DEPTH LIMITS BELOW 16.  The blobs and the packers take D = 2..16; three launches keep D-proportional tables beside the 96 KiB weight ring
// in the CU's 160 KiB of LDS and run out of it sooner (each launcher static_asserts its own formula against these):
//   split-precision forward (mlp_f16s_kernel, inference and stash): side tables with D x 256 biases + 34 KiB of per-wave buffers   D <= 14
//   bf16 / f16 forward, 64 points per wave: the same side tables + 36 KiB of per-wave buffers (32 points per wave: 18 KiB)         D <= 12
//   split-precision backward data (dgrad_f16s_kernel): 4 KiB of ReLU' words per layer                                               D <= 15
constexpr int LDS_BYTES = 160 * 1024;
constexpr int F16S_FWD_MAX_D = 14, HALF_64PT_MAX_D = 12, F16S_DGRAD_MAX_D = 15;
__host__ __device__ constexpr size_t half_side_bytes(int D) { return ((size_t)D * 256 + 256 + 128 + 4 + (3 + 6 * KERNEL_LD) * 128) * 4; }

// shapes the 16-bit variants are built for; `variant`: "bf16", "f16-split", "f16"
inline int check_net_half(const mi_nerf_net* net, const char* variant) {
    MN_CHECK_ARG(net != nullptr, "net is NULL");
    MN_CHECK_ARG(net->W == 256, "the %s variant is built for W=256 only (got %d; weights.PackedNeRF pads narrower networks)", variant, net->W);
    MN_CHECK_ARG(net->D >= 2 && net->D <= 16 && net->L_x >= 0 && net->L_x <= KERNEL_LX && net->L_d >= 0 && net->L_d <= KERNEL_LD && net->skip >= -1,
                 "unsupported network for the %s variant (D=%d L_x=%d L_d=%d skip=%d)", variant, net->D, net->L_x, net->L_d, net->skip);
    return MI_NERF_OK;
}
// ... and the split-precision FORWARD on top of it (inference, training forward, every render mode whose plan has an F16S family): checked
// before the first launch of a render, not when the launch is reached
inline int check_net_f16s_forward(const mi_nerf_net* net) {
    if (int rc = check_net_half(net, "f16-split")) return rc;
    MN_CHECK_ARG(net->D <= F16S_FWD_MAX_D, "the split-precision forward kernel keeps every layer's biases and its waves' encoding buffers beside the weight ring in LDS: "
                 "D = %d does not fit (D <= %d); a deeper network runs in fp32, bf16 or f16", net->D, F16S_FWD_MAX_D);
    return MI_NERF_OK;
}

// A parameter set whose values are their own flat index + 1 (module.parameters() order: layout.h make_param_offsets; exact in fp32 below
// 2^24).  A host packer run over it writes, at every blob position, which parameter feeds it (0: constant zero): the gather maps of the
// device-side packers.  `p` points into `flat`.
struct IndexParams {
    std::vector<float> flat;
    std::vector<const float*> wx, bx;
    mi_nerf_params p;
};
int make_index_params(const mi_nerf_net* net, IndexParams& ip);      // pack.cpp

// ---- packer entry points (api.hip calls these) --------------------------------------------------------------------------------------------
// pack.cpp: the fp32 blobs
int pack_fp32(const mi_nerf_net*, const mi_nerf_params*, void* blob, size_t blob_bytes);
size_t packed_bytes_bwd(const mi_nerf_net*);
int pack_bwd_fp32(const mi_nerf_net*, const mi_nerf_params*, void* blob, size_t blob_bytes);
int pack_map(const mi_nerf_net*, int kind, int32_t* map, size_t map_len);
// pack_half.hip: per 16-bit kind the blob size, the host packer, the gather map (length in entries) and the device-side packer over that map;
// bad_dev (may be NULL): device counter of stream elements whose weight is NaN or beyond the f16 range
size_t packed_bytes_bf16(const mi_nerf_net*);
int pack_bf16(const mi_nerf_net*, const mi_nerf_params*, void* blob, size_t blob_bytes);
size_t pack_map_bf16_len(const mi_nerf_net*);
int pack_map_bf16(const mi_nerf_net*, int32_t* map, size_t map_len);
int pack_apply_bf16(const mi_nerf_net*, const int32_t* map_dev, const float* flat_dev, void* blob_dev, size_t blob_bytes, hipStream_t);
size_t packed_bytes_f16s(const mi_nerf_net*);
int pack_f16s(const mi_nerf_net*, const mi_nerf_params*, void* blob, size_t blob_bytes);
size_t pack_map_f16s_len(const mi_nerf_net*);
int pack_map_f16s(const mi_nerf_net*, int32_t* map, size_t map_len);
int pack_apply_f16s(const mi_nerf_net*, const int32_t* map_dev, const float* flat_dev, void* blob_dev, size_t blob_bytes, unsigned* bad_dev, hipStream_t);
size_t packed_bytes_bwd_f16s(const mi_nerf_net*);
int pack_bwd_f16s(const mi_nerf_net*, const mi_nerf_params*, void* blob, size_t blob_bytes);
size_t pack_map_bwd_f16s_len(const mi_nerf_net*);
int pack_map_bwd_f16s(const mi_nerf_net*, int32_t* map, size_t map_len);
int pack_apply_bwd_f16s(const mi_nerf_net*, const int32_t* map_dev, const float* flat_dev, void* blob_dev, size_t blob_bytes, unsigned* bad_dev, hipStream_t);

}  // namespace minerf
