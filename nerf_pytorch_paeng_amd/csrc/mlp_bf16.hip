// mlp_bf16.hip -- bf16-MFMA variant of the fused positional-encoding + NeRF MLP forward (BASELINE config #5).
//
// Same idea as mlp_fp32.hip -- activations never leave registers, the accumulator of layer l becomes the B operand of
// layer l+1, weights stream L2 -> LDS in consumption order -- rebuilt around what bf16 MFMA makes expensive: at 16x the
// fp32 MFMA rate a 256-wide layer is only 4096 matrix cycles per 32 points, so everything that is NOT an MFMA
// (accumulator -> bf16 packing, biases, gamma(x), heads), the weight stream and -- above all -- the POWER the chip
// has to spend per FLOP decide the speed.  (Round 1's kernel, with the fp32 kernel's k-outer order: 5.8 VALU
// instructions per MFMA, all exposed at the layer boundaries; 7.5 GB of L2 -> LDS weight traffic per launch; 42 % MFMA
// busy at 2.0 GHz -- profiles/r02_bf16_old_pmc*.json.)
//
//   * OUTPUT-TILE-MAJOR order ("t-outer").  A layer is 16 jobs; job t computes output features 16t..16t+15 over ALL
//     k-steps with ONE small accumulator per point tile.  Tiles 2s, 2s+1 of layer l are exactly B fragment s of layer
//     l+1, which that layer does not touch before its k-step s -- so the packing of job j's accumulators
//     (v_cvt_pk_bf16_f32 + ReLU as v_pk_max_i16 on the packed pair) is dealt out over the groups of job j+1, across
//     layer boundaries as well: there IS no layer boundary.  The bias is the C operand of a job's first MFMA.
//   * 64 POINTS PER WAVE (four point tiles of 16, one wave per SIMD): every A fragment (one ds_read_b128 per lane)
//     feeds four MFMAs (64 matrix cycles), so LDS reads and the L2 -> LDS stream are half of the 32-points-per-wave
//     design per FLOP (256 points per workgroup per pass over the 1.2 MB stream).  A second instantiation with 32 points
//     per wave (NP = 2) serves launches too small to give every SIMD a 64-point unit (see NP below).
//   * v_mfma_f32_16x16x32_bf16, not 32x32x16: the kernel is POWER limited (a build stripped to MFMAs + A-fragment
//     reads runs at ~1.7 GHz, profiles/r02_bf16_ablation.json), and at equal cycles per FLOP the chip holds a higher
//     clock on the 16x16x32 shape (tools/mfma_probe4.hip: +9 % FLOP/s for this operand pattern; MI355X_MICROARCH.md,
//     DVFS give-back item 7).  It also quarters the accumulator registers (4 per tile instead of 16).
//   * THE FRAGMENT FILE: both ping-pong sets of B fragments (2 x 4 point tiles x 8 fragments x 4 registers = all 256
//     AGPRs) are managed by hand with explicit register numbers; hipcc allocates only the VGPR side (see below).
//   * HEADS ON THE MATRIX PIPE.  Density (256 -> 1) is row 3 of an extra 16-row output tile over the trunk output (8
//     k-steps, right after the feature layer), colour (128 -> 3) rows 0..2 of another over the view-direction layer's
//     output (4 k-steps): (r, g, b) and the density land in registers 0..2 / 3 of lanes 0..15, one 16-byte store per
//     point; no VALU dot products, no cross-lane shuffles.  (+1 % MFMAs, -500 VALU per 32 points.)
//   * gamma(x) by ANGLE DOUBLING: one accurate sin/cos per axis (Cody-Waite + Cephes, as the fp32 kernel), then
//     s' = 2sc, c' = 1 - 2s^2 for the nine higher octaves.  The recurrence doubles the error per octave (<= 2^9 * 1e-7 =
//     5e-5 at the top octave), two orders below the bf16 rounding (2^-9 relative) the values get next.  The fp32
//     kernel keeps one full-precision evaluation per channel; this is the bf16 variant's own accuracy contract
//     (checked against an oracle with the same rounding points, and as PSNR against the fp32 path).
//
//   * SMALL COARSE LAUNCHES DO render_rays' MIDDLE THEMSELVES (round 6).  One 32-point unit per wave and 33..64 coarse samples = two units per
//     ray: a workgroup's four waves hold two rays whole, so its epilogue composites them and draws their fine depths (composite_ray +
//     fine_z_ray of stage_dev.h -- the stage kernel's own device functions: bit-identical) and mi_nerf_render_rays skips that launch:
//     -2.2 us of a ~125 us step at the 512-ray shard of an 8-GPU split (profiles/r06_bf16_fused_stages_ab.txt).  From 513 to 1024 rays a wave's
//     one 64-point unit IS a ray, and every wave does the middle for its own ray (-1.8 us of ~205 at 1024 rays).
//
//   A fragment: lane l (i = l&15, q = l>>4) holds A[i][k = 8q + j], j = 0..7  (8 bf16 = 16 B = one ds_read_b128)
//   B fragment: lane l holds B[k = 8q + j][col = l&15]
//   D (4 registers): col = l&15, row = 4q + r
// so the accumulators of output tiles 2s (elements j = 0..3) and 2s+1 (j = 4..7), packed pairwise, are the B fragment of
// k-step s whose element j on lane quarter q is feature 16(2s + (j>>2)) + 4q + (j&3); the weights are packed in that
// order on the host.  Encoded inputs: slot u = 32 ks + 8q + j is channel u of gamma(x) (zero weight beyond the last).
//
// Stream (1 KiB quads = the A fragment of FOUR MFMAs; 32 KiB slots, 3-slot ring, LDS-DMA two slots ahead):
//   layer 0:   for T in 0..15: 2 gamma(x) k-steps                                   32 quads
//   layer l:   for T in 0..15: 8 activation k-steps [2 gamma(x) k-steps if skip]    128 | 160 quads
//   tail:      feature layer (16 x 8) | density tile over the trunk output (8) | view-direction layer (8 x 8)
//              | colour tile over the view-direction output (4) | 20 quads of padding   224 quads
#include "mlp_half_core.h"

namespace minerf {


struct BlobLayoutBf16 {
    uint32_t stream_off, stream_bytes, side_off, side_floats;
    uint32_t bias_trunk, bias_feat, bias_d, head_b, wdir_t, total_bytes;
};

static BlobLayoutBf16 make_layout_bf16(int D, int W, int skip, int /*L_x*/, int /*L_d*/) {
    constexpr int L_x = KERNEL_LX, L_d = KERNEL_LD;          // the kernel's layout; a network with fewer frequencies gets zero weights (layout.h)
    BlobLayoutBf16 b{};
    const int NT = W / MT, in_d = 3 + 6 * L_d;
    const uint32_t pe_q = (uint32_t)enc_ksteps32(L_x) * NT, h_q = (uint32_t)(W / KF) * NT;
    uint32_t quads = pe_q;
    for (int l = 1; l < D; ++l) quads += h_q + ((skip >= 0 && l == skip + 1) ? pe_q : 0);
    quads += TAIL_QUADS;
    b.stream_off = HEADER_BYTES;
    b.stream_bytes = quads * QUAD_BYTES;
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

// ---------------------------------------------------------------------------------------------
// host: packer
// ---------------------------------------------------------------------------------------------
static inline uint16_t f32_to_bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);      // NaN stays NaN
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// The stream is emitted either as bf16 (the blob) or as the float itself (the gather map of the device-side packer, built by
// running this packer over parameters whose values are their own flat index + 1).
template <typename T> static inline T stream_elem(float x);
template <> inline uint16_t stream_elem<uint16_t>(float x) { return f32_to_bf16_rne(x); }
template <> inline float stream_elem<float>(float x) { return x; }

// One quad: the A fragment of output rows row0..row0+15 for the 32 input columns cols[q*8 + j] (-1: zero).
// rowmap (optional, 16 entries): weight-matrix row feeding output row i of the tile, -1: zero row.
template <typename T>
static void emit_quad(std::vector<T>& st, const float* Wm, int n_out, int n_in, int row0, const int* rowmap, const int* cols) {
    for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
            const int col = cols[(lane >> 4) * 8 + j];
            const int n = rowmap ? rowmap[lane & 15] : row0 + (lane & 15);
            st.push_back((col >= 0 && n >= 0 && n < n_out) ? stream_elem<T>(Wm[(size_t)n * n_in + col]) : (T)0);
        }
}
static std::vector<int> enc_cols32(int L, int base) {           // L: the network's own frequencies; the k-step count is the kernel's
    const int nch = 3 + 6 * L, KS = enc_ksteps32(KERNEL_LX);
    std::vector<int> c(KS * KF);
    for (int u = 0; u < KS * KF; ++u) c[u] = u < nch ? base + u : -1;
    return c;
}
// input columns in the order the packed accumulators present them: fragment s, lane quarter q, element j
static std::vector<int> act_cols32(int W, int base) {
    std::vector<int> c;
    for (int s = 0; s < W / KF; ++s)
        for (int q = 0; q < 4; ++q)
            for (int j = 0; j < 8; ++j) c.push_back(base + MT * (2 * s + (j >> 2)) + 4 * q + (j & 3));
    return c;
}
// a layer in output-tile-major order: for every tile, all its k-steps
template <typename T>
static void emit_layer(std::vector<T>& st, const float* Wm, int n_out, int n_in, int NT, const std::vector<int>& cols) {
    const int KS = (int)cols.size() / KF;
    for (int tile = 0; tile < NT; ++tile)
        for (int ks = 0; ks < KS; ++ks) emit_quad(st, Wm, n_out, n_in, MT * tile, nullptr, cols.data() + KF * ks);
}

static int check_net_bf16(const mi_nerf_net* net) {
    MN_CHECK_ARG(net != nullptr, "net is NULL");
    MN_CHECK_ARG(net->W == 256, "the bf16 variant is built for W=256 only (got %d)", net->W);
    MN_CHECK_ARG(net->D >= 2 && net->D <= 16 && net->L_x >= 0 && net->L_x <= KERNEL_LX && net->L_d >= 0 && net->L_d <= KERNEL_LD && net->skip >= -1,
                 "unsupported network for bf16 (D=%d L_x=%d L_d=%d skip=%d)", net->D, net->L_x, net->L_d, net->skip);
    return MI_NERF_OK;
}

size_t packed_bytes_bf16(const mi_nerf_net* net) {
    if (check_net_bf16(net)) return 0;
    return make_layout_bf16(net->D, net->W, net->skip, net->L_x, net->L_d).total_bytes;
}

// the weight stream in consumption order
template <typename T>
static int build_stream(const mi_nerf_net* net, const mi_nerf_params* p, const BlobLayoutBf16& L, std::vector<T>& st) {
    const int D = net->D, W = net->W, NT = W / MT;
    const int in_x = 3 + 6 * net->L_x, in_d = 3 + 6 * net->L_d;
    const size_t per_quad = QUAD_BYTES / 2;
    st.reserve(L.stream_bytes / 2);
    emit_layer(st, p->linear_x_w[0], W, in_x, NT, enc_cols32(net->L_x, 0));
    for (int l = 1; l < D; ++l) {
        const bool cat = (net->skip >= 0 && l == net->skip + 1);
        std::vector<int> cols = act_cols32(W, cat ? in_x : 0);          // input columns are cat([gamma(x), h]), NeRF.py:41 ...
        if (cat) {                                                      // ... consumed activations first, gamma(x) last
            const std::vector<int> enc = enc_cols32(net->L_x, 0);
            cols.insert(cols.end(), enc.begin(), enc.end());
        }
        emit_layer(st, p->linear_x_w[l], W, cat ? W + in_x : W, NT, cols);
    }
    // tail: feature layer | density tile over the trunk output | view-direction layer | colour tile
    emit_layer(st, p->linear_feat_w, W, W, NT, act_cols32(W, 0));
    int rowmap[MT];
    {
        const std::vector<int> act = act_cols32(W, 0);
        for (int i = 0; i < MT; ++i) rowmap[i] = (i == 3) ? 0 : -1;     // output row 3 <- linear_density row 0
        for (int ks = 0; ks < W / KF; ++ks) emit_quad(st, p->linear_density_w, 1, W, 0, rowmap, act.data() + KF * ks);
    }
    emit_layer(st, p->linear_d_w, W / 2, W + in_d, NT / 2, act_cols32(W, 0));
    {
        const std::vector<int> act = act_cols32(W / 2, 0);
        for (int i = 0; i < MT; ++i) rowmap[i] = (i < 3) ? i : -1;      // output rows 0..2 <- linear_color rows 0..2
        for (int ks = 0; ks < W / 2 / KF; ++ks) emit_quad(st, p->linear_color_w, 3, W / 2, 0, rowmap, act.data() + KF * ks);
    }
    st.resize(st.size() + (size_t)(TAIL_QUADS - TAIL_USED) * per_quad, (T)0);
    MN_CHECK_ARG(st.size() * 2 == L.stream_bytes, "internal: bf16 stream %zu != %u", st.size() * 2, L.stream_bytes);
    return MI_NERF_OK;
}
// the fp32 side tables
static void fill_side(const mi_nerf_net* net, const mi_nerf_params* p, const BlobLayoutBf16& L, float* side) {
    const int D = net->D, W = net->W, in_d = 3 + 6 * net->L_d;
    for (int l = 0; l < D; ++l) memcpy(side + L.bias_trunk + (size_t)l * W, p->linear_x_b[l], W * 4);
    memcpy(side + L.bias_feat, p->linear_feat_b, W * 4);
    memcpy(side + L.bias_d, p->linear_d_b, (W / 2) * 4);
    memcpy(side + L.head_b, p->linear_color_b, 3 * 4);
    side[L.head_b + 3] = p->linear_density_b[0];
    for (int f = 0; f < in_d; ++f)
        for (int n = 0; n < W / 2; ++n) side[L.wdir_t + (size_t)f * (W / 2) + n] = p->linear_d_w[(size_t)n * (W + in_d) + W + f];
}
static void fill_header(const mi_nerf_net* net, const BlobLayoutBf16& L, uint32_t* hdr) {
    memset(hdr, 0, HEADER_BYTES);
    hdr[0] = BLOB_MAGIC; hdr[1] = 3; hdr[2] = net->D; hdr[3] = net->W; hdr[4] = (uint32_t)net->skip; hdr[5] = KERNEL_LX; hdr[6] = KERNEL_LD;   // the layout's
    hdr[13] = net->L_x; hdr[14] = net->L_d;                                                                                                    // the network's
    hdr[7] = L.stream_off; hdr[8] = L.stream_bytes; hdr[9] = L.stream_bytes; hdr[10] = L.side_off; hdr[11] = L.side_floats;
    hdr[12] = 2;   // stream element bytes
}

int pack_bf16(const mi_nerf_net* net, const mi_nerf_params* p, void* blob, size_t blob_bytes) {
    if (int rc = check_net_bf16(net)) return rc;
    const BlobLayoutBf16 L = make_layout_bf16(net->D, net->W, net->skip, net->L_x, net->L_d);
    MN_CHECK_ARG(blob_bytes >= L.total_bytes, "blob too small: %zu < %u", blob_bytes, L.total_bytes);
    memset(blob, 0, L.total_bytes);
    std::vector<uint16_t> st;
    if (int rc = build_stream(net, p, L, st)) return rc;
    fill_header(net, L, (uint32_t*)blob);
    memcpy((char*)blob + L.stream_off, st.data(), L.stream_bytes);
    fill_side(net, p, L, (float*)((char*)blob + L.side_off));
    return MI_NERF_OK;
}

// Device-side packing of the bf16 blob (a model whose parameters live on the device is re-packed for every call: weights.py):
// gather map from the flat parameter vector (mi_nerf_param_count order), one entry per stream ELEMENT followed by one per side
// float; entry = 1 + flat index, 0 = constant zero.  Built like pack_map (pack.cpp): this packer run over index-valued parameters.
size_t pack_map_bf16_len(const mi_nerf_net* net) {
    if (check_net_bf16(net)) return 0;
    const BlobLayoutBf16 L = make_layout_bf16(net->D, net->W, net->skip, net->L_x, net->L_d);
    return (size_t)L.stream_bytes / 2 + L.side_floats;
}
int pack_map_bf16(const mi_nerf_net* net, int32_t* map, size_t map_len) {
    if (int rc = check_net_bf16(net)) return rc;
    const int D = net->D, W = net->W;
    const BlobLayoutBf16 L = make_layout_bf16(D, W, net->skip, net->L_x, net->L_d);
    const ParamOffsets po = make_param_offsets(D, W, net->skip, net->L_x, net->L_d);
    MN_CHECK_ARG(po.total < (1u << 24), "network too large for the index map (%u parameters)", po.total);
    const size_t n_stream = (size_t)L.stream_bytes / 2;
    MN_CHECK_ARG(map && map_len >= n_stream + L.side_floats, "map too small: %zu entries for %zu", map_len, n_stream + L.side_floats);
    std::vector<float> flat(po.total);
    for (uint32_t i = 0; i < po.total; ++i) flat[i] = (float)(i + 1);
    std::vector<const float*> wx(D), bx(D);
    for (int l = 0; l < D; ++l) { wx[l] = flat.data() + po.w_x[l]; bx[l] = flat.data() + po.b_x[l]; }
    mi_nerf_params p{};
    p.linear_x_w = wx.data(); p.linear_x_b = bx.data();
    p.linear_density_w = flat.data() + po.w_dens; p.linear_density_b = flat.data() + po.b_dens;
    p.linear_feat_w = flat.data() + po.w_feat; p.linear_feat_b = flat.data() + po.b_feat;
    p.linear_d_w = flat.data() + po.w_d; p.linear_d_b = flat.data() + po.b_d;
    p.linear_color_w = flat.data() + po.w_color; p.linear_color_b = flat.data() + po.b_color;
    std::vector<float> st;
    if (int rc = build_stream(net, &p, L, st)) return rc;
    std::vector<float> side(L.side_floats, 0.0f);
    fill_side(net, &p, L, side.data());
    for (size_t i = 0; i < n_stream; ++i) map[i] = (int32_t)st[i];
    for (size_t i = 0; i < L.side_floats; ++i) map[n_stream + i] = (int32_t)side[i];
    return MI_NERF_OK;
}

struct HeaderWords { uint32_t w[HEADER_BYTES / 4]; };
__global__ __launch_bounds__(256) void pack_apply_bf16_kernel(const int32_t* __restrict__ map, const float* __restrict__ flat, unsigned n_stream,
                                                               unsigned n_side, unsigned stream_off, unsigned side_off, HeaderWords hdr,
                                                               char* __restrict__ blob) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < HEADER_BYTES / 4) ((uint32_t*)blob)[i] = hdr.w[i];
    if (i < n_stream) {
        const int32_t m = map[i];
        unsigned u = m ? __float_as_uint(flat[m - 1]) : 0u;
        u = ((u & 0x7FFFFFFFu) > 0x7F800000u) ? ((u >> 16) | 0x40u) : ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);      // f32_to_bf16_rne
        ((uint16_t*)(blob + stream_off))[i] = (uint16_t)u;
    } else if (i < n_stream + n_side) {
        const int32_t m = map[i];
        ((float*)(blob + side_off))[i - n_stream] = m ? flat[m - 1] : 0.0f;
    }
}
int pack_apply_bf16(const mi_nerf_net* net, const int32_t* map_dev, const float* flat_dev, void* blob_dev, size_t blob_bytes, hipStream_t st) {
    if (int rc = check_net_bf16(net)) return rc;
    const BlobLayoutBf16 L = make_layout_bf16(net->D, net->W, net->skip, net->L_x, net->L_d);
    MN_CHECK_ARG(map_dev && flat_dev && blob_dev, "NULL device pointer");
    MN_CHECK_ARG(blob_bytes >= L.total_bytes && ((uintptr_t)blob_dev & 15) == 0, "blob too small (%zu < %u) or not 16-byte aligned", blob_bytes, L.total_bytes);
    HeaderWords h;
    fill_header(net, L, h.w);
    const unsigned n_stream = L.stream_bytes / 2, total = n_stream + L.side_floats;
    hipLaunchKernelGGL(pack_apply_bf16_kernel, dim3((total + 255) / 256), dim3(256), 0, st, map_dev, flat_dev, n_stream, L.side_floats, L.stream_off,
                       L.side_off, h, (char*)blob_dev);
    MN_LAUNCH_CHECK("pack_apply_bf16_kernel");
    return MI_NERF_OK;
}


int mlp_rays_bf16(const mi_nerf_net* net, const void* packed_dev, const float* rays_dev, const float* z_dev, int64_t n_rays, int S,
                  float* raw_dev, hipStream_t st, int points_per_wave, const StratDraw* strat, FineDraw* fine) {
    if (fine) fine->taken = false;
    if (int rc = check_net_bf16(net)) return rc;
    const BlobLayoutBf16 b = make_layout_bf16(net->D, net->W, net->skip, net->L_x, net->L_d);
    const HalfBlob L{b.stream_off, b.stream_bytes, b.side_off, b.side_floats, b.bias_trunk, b.bias_feat, b.bias_d, b.head_b, b.wdir_t};
    return mlp_rays_half<false>(net, L, packed_dev, rays_dev, z_dev, n_rays, S, raw_dev, st, points_per_wave, strat, fine);
}

}  // namespace minerf
