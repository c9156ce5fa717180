// pack_half.hip -- the packers of the 16-bit weight blobs (half_layout.h: bf16, split-precision forward, split-precision backward):
// reference checkpoint layout -> the stream order of the 16x16x32 kernels, on the host (once per checkpoint) and on the device (a model
// whose parameters live there is re-packed for every call, the training path after every optimizer step: weights.py, train_path.py).
//
// Every packer is the same three steps:
//   1. the blob's VALUES in blob order -- one float per 16-bit stream element, then the fp32 side tables.  A split-precision position
//      holds the source weight twice, at its hi and at its lo element (element i of a 1024-element pair block is a hi half for i < 512);
//   2. a FINISHER per element: round to bf16 | the hi or lo half of the f16 split (refusing |w| >= 65504 and NaN) | the value as int32;
//   3. the header.
// Run over index-valued parameters (make_index_params) with the int32 finisher, steps 1 and 2 give the gather map of the device-side
// packer: map[i] = 1 + flat parameter index feeding blob element i, 0 = constant zero.  pack_apply_half_kernel is steps 2 and 3 on the
// device over that map.  The stream order itself is described in mlp_bf16.hip (forward) and dgrad_f16s.hip (backward chain).
#include <string.h>
#include "half_layout.h"

namespace minerf {

enum BlobKind { KIND_BF16 = 3, KIND_F16S = 4, KIND_F16S_BWD = 5 };      // header word 1
struct HeaderWords { uint32_t w[HEADER_BYTES / 4]; };

namespace {

constexpr int QUAD_ELEMS = QUAD_BYTES / 2;

// ---------------------------------------------------------------------------------------------
// element finishers
// ---------------------------------------------------------------------------------------------
inline uint16_t f32_to_bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);      // NaN stays NaN
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
inline uint16_t f32_to_f16_rne(float x) {            // finite |x| < 65520 (checked by the caller)
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);                           // >= 65536: inf (not reached)
    if (a < 0x38800000u) {                                                              // below 2^-14: subnormal half (or zero)
        if (a < 0x33000000u) return (uint16_t)sign;                                     // below 2^-25: zero
        const uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
        const int shift = 126 - (int)(a >> 23);                                         // 14 .. 24
        const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
    }
    const uint32_t r = a + 0xFFFu + ((a >> 13) & 1u);                                   // round to nearest even at bit 13
    return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}
inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = sign;
        else { int k = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; ++k; } u = sign | ((uint32_t)(113 - k) << 23) | ((mm & 0x3FFu) << 13); }
    } else if (e == 31) u = sign | 0x7F800000u | (m << 13);
    else u = sign | ((e + 112u) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// stream element i of a split-precision blob: the hi or the lo half of w = hi + lo * 2^-11
inline uint16_t split_elem(float w, size_t i) {
    const uint16_t hi = f32_to_f16_rne(w);
    return (i & (2 * QUAD_ELEMS - 1)) < (size_t)QUAD_ELEMS ? hi : f32_to_f16_rne((w - f16_to_f32(hi)) * SPLIT_SCALE);
}
inline bool fits_f16(float w) { return w == w && (w < 0 ? -w : w) < 65504.0f; }
int check_weights(const float* w, size_t n, const char* name) {
    for (size_t i = 0; i < n; ++i) MN_CHECK_ARG(fits_f16(w[i]), "%s[%zu] = %g does not fit the f16-split variant", name, i, (double)w[i]);
    return MI_NERF_OK;
}

// ---------------------------------------------------------------------------------------------
// value streams
// ---------------------------------------------------------------------------------------------
// One stream position: `copies` quads (1: bf16, 2: a (hi, lo) pair), each the A fragment of 16 output rows x 32 k columns -- lane l
// (i = l & 15, q = l >> 4), element j holds at(i, 8q + j)  (mlp_bf16.hip "A fragment").
template <typename At>
void emit_pos(std::vector<float>& st, int copies, At at) {
    const size_t base = st.size();
    st.resize(base + (size_t)copies * QUAD_ELEMS, 0.0f);
    for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
            const float w = at(lane & 15, (lane >> 4) * 8 + j);
            for (int c = 0; c < copies; ++c) st[base + (size_t)c * QUAD_ELEMS + lane * 8 + j] = w;
        }
}
// forward GEMM: output rows row0..row0+15 of Wm [n_out, n_in] for the 32 input columns cols[k] (-1: zero).
// rowmap (optional, 16 entries): weight-matrix row feeding output row i of the tile, -1: zero row.
void emit_fwd(std::vector<float>& st, int copies, const float* Wm, int n_out, int n_in, int row0, const int* rowmap, const int* cols) {
    emit_pos(st, copies, [=](int i, int k) {
        const int col = cols[k], n = rowmap ? rowmap[i] : row0 + i;
        return (col >= 0 && n >= 0 && n < n_out) ? Wm[(size_t)n * n_in + col] : 0.0f;
    });
}
// transposed GEMM: output rows = forward INPUT columns in_base + row0 .. +15, k = forward OUTPUT rows cols[k] (-1: zero)
void emit_bwd(std::vector<float>& st, int copies, const float* Wm, int n_out_fwd, int n_in_fwd, int in_base, int row0, const int* cols) {
    emit_pos(st, copies, [=](int i, int k) {
        const int col = cols[k], n = in_base + row0 + i;
        return (col >= 0 && col < n_out_fwd && n < n_in_fwd) ? Wm[(size_t)col * n_in_fwd + n] : 0.0f;
    });
}
std::vector<int> enc_cols(int L, int base) {           // L: the network's own frequencies; the k-step count is the kernel's
    const int nch = 3 + 6 * L, n = enc_ksteps32(KERNEL_LX) * KF;
    std::vector<int> c(n);
    for (int u = 0; u < n; ++u) c[u] = u < nch ? base + u : -1;
    return c;
}
// input columns in the order the packed accumulators present them: fragment s, lane quarter q, element j
std::vector<int> act_cols(int W, int base) {
    std::vector<int> c;
    for (int s = 0; s < W / KF; ++s)
        for (int q = 0; q < 4; ++q)
            for (int j = 0; j < 8; ++j) c.push_back(base + MT * (2 * s + (j >> 2)) + 4 * q + (j & 3));
    return c;
}
// a layer in output-tile-major order: for every tile, all its k-steps
void layer_fwd(std::vector<float>& st, int copies, const float* Wm, int n_out, int n_in, int NT, const std::vector<int>& cols) {
    const int KS = (int)cols.size() / KF;
    for (int tile = 0; tile < NT; ++tile)
        for (int ks = 0; ks < KS; ++ks) emit_fwd(st, copies, Wm, n_out, n_in, MT * tile, nullptr, cols.data() + KF * ks);
}
void layer_bwd(std::vector<float>& st, int copies, const float* Wm, int n_out_fwd, int n_in_fwd, int in_base, int NT, const std::vector<int>& cols) {
    const int KS = (int)cols.size() / KF;
    for (int tile = 0; tile < NT; ++tile)
        for (int ks = 0; ks < KS; ++ks) emit_bwd(st, copies, Wm, n_out_fwd, n_in_fwd, in_base, MT * tile, cols.data() + KF * ks);
}

// the forward stream in consumption order
void stream_fwd(const mi_nerf_net* net, const mi_nerf_params* p, int copies, std::vector<float>& st) {
    const int D = net->D, W = net->W, NT = W / MT;
    const int in_x = 3 + 6 * net->L_x, in_d = 3 + 6 * net->L_d;
    layer_fwd(st, copies, p->linear_x_w[0], W, in_x, NT, enc_cols(net->L_x, 0));
    for (int l = 1; l < D; ++l) {
        const bool cat = (net->skip >= 0 && l == net->skip + 1);
        std::vector<int> cols = act_cols(W, cat ? in_x : 0);            // input columns are cat([gamma(x), h]), NeRF.py:41 ...
        if (cat) {                                                      // ... consumed activations first, gamma(x) last
            const std::vector<int> enc = enc_cols(net->L_x, 0);
            cols.insert(cols.end(), enc.begin(), enc.end());
        }
        layer_fwd(st, copies, p->linear_x_w[l], W, cat ? W + in_x : W, NT, cols);
    }
    // tail: feature layer | density tile over the trunk output | view-direction layer | colour tile | padding
    layer_fwd(st, copies, p->linear_feat_w, W, W, NT, act_cols(W, 0));
    int rowmap[MT];
    {
        const std::vector<int> act = act_cols(W, 0);
        for (int i = 0; i < MT; ++i) rowmap[i] = (i == 3) ? 0 : -1;     // output row 3 <- linear_density row 0
        for (int ks = 0; ks < W / KF; ++ks) emit_fwd(st, copies, p->linear_density_w, 1, W, 0, rowmap, act.data() + KF * ks);
    }
    layer_fwd(st, copies, p->linear_d_w, W / 2, W + in_d, NT / 2, act_cols(W, 0));
    {
        const std::vector<int> act = act_cols(W / 2, 0);
        for (int i = 0; i < MT; ++i) rowmap[i] = (i < 3) ? i : -1;      // output rows 0..2 <- linear_color rows 0..2
        for (int ks = 0; ks < W / 2 / KF; ++ks) emit_fwd(st, copies, p->linear_color_w, 3, W / 2, 0, rowmap, act.data() + KF * ks);
    }
    st.resize(st.size() + (size_t)((copies == 2 ? TAIL_PAIRS : TAIL_QUADS) - TAIL_USED) * copies * QUAD_ELEMS, 0.0f);
}
// the backward-data stream: the TRANSPOSED weights in the order the chain
//   d hidden -> linear_d^T (feature block) -> linear_feat^T -> linear_x[D-1]^T ... linear_x[1]^T (activation block)
// consumes them (pack.cpp pack_bwd_fp32 is the fp32 counterpart).  The colour / density head weights are read from the fp32 forward
// blob's side tables like mlp_dgrad_kernel does.
void stream_bwd(const mi_nerf_net* net, const mi_nerf_params* p, int copies, std::vector<float>& st) {
    const int D = net->D, W = net->W, NT = W / MT;
    const int in_x = 3 + 6 * net->L_x, in_d = 3 + 6 * net->L_d;
    layer_bwd(st, copies, p->linear_d_w, W / 2, W + in_d, 0, NT, act_cols(W / 2, 0));         // d feature = Wd[:, :W]^T d hidden
    layer_bwd(st, copies, p->linear_feat_w, W, W, 0, NT, act_cols(W, 0));
    for (int l = D - 1; l >= 1; --l) {
        const bool cat = (net->skip >= 0 && l == net->skip + 1);
        layer_bwd(st, copies, p->linear_x_w[l], W, cat ? W + in_x : W, cat ? in_x : 0, NT, act_cols(W, 0));
    }
}
// the fp32 side tables
void fill_side(const mi_nerf_net* net, const mi_nerf_params* p, const HalfLayout& L, float* side) {
    const int D = net->D, W = net->W, in_d = 3 + 6 * net->L_d;
    for (int l = 0; l < D; ++l) memcpy(side + L.bias_trunk + (size_t)l * W, p->linear_x_b[l], W * 4);
    memcpy(side + L.bias_feat, p->linear_feat_b, W * 4);
    memcpy(side + L.bias_d, p->linear_d_b, (W / 2) * 4);
    memcpy(side + L.head_b, p->linear_color_b, 3 * 4);
    side[L.head_b + 3] = p->linear_density_b[0];
    for (int f = 0; f < in_d; ++f)
        for (int n = 0; n < W / 2; ++n) side[L.wdir_t + (size_t)f * (W / 2) + n] = p->linear_d_w[(size_t)n * (W + in_d) + W + f];
}
void fill_header(const mi_nerf_net* net, int kind, const HalfLayout& L, uint32_t* hdr) {
    memset(hdr, 0, HEADER_BYTES);
    hdr[0] = BLOB_MAGIC; hdr[1] = (uint32_t)kind; hdr[2] = net->D; hdr[3] = net->W; hdr[4] = (uint32_t)net->skip;
    hdr[7] = L.stream_off; hdr[8] = L.stream_bytes;
    if (kind == KIND_F16S_BWD) { hdr[5] = net->L_x; hdr[6] = net->L_d; return; }
    hdr[5] = KERNEL_LX; hdr[6] = KERNEL_LD;                     // the layout's
    hdr[13] = net->L_x; hdr[14] = net->L_d;                     // the network's
    hdr[9] = L.stream_bytes; hdr[10] = L.side_off; hdr[11] = L.side_floats;
    hdr[12] = 2;   // stream element bytes
}

// ---------------------------------------------------------------------------------------------
// the three steps, per blob kind
// ---------------------------------------------------------------------------------------------
// the network check and the blob's extent; the backward blob is header | stream (no side tables: side_off == total_bytes)
int blob_layout(const mi_nerf_net* net, int kind, HalfLayout* L) {
    if (int rc = check_net_half(net, kind == KIND_BF16 ? "bf16" : "f16-split")) return rc;
    if (kind == KIND_F16S_BWD) {
        *L = HalfLayout{};
        L->stream_off = HEADER_BYTES;
        L->stream_bytes = bwd_stream_bytes_s(net->D);
        L->side_off = L->total_bytes = L->stream_off + L->stream_bytes;
    } else {
        *L = make_half_layout(net->D, net->W, net->skip, kind == KIND_BF16 ? HalfStream::QUADS : HalfStream::PAIRS);
    }
    return MI_NERF_OK;
}
size_t blob_bytes_of(const mi_nerf_net* net, int kind) {
    HalfLayout L;
    return blob_layout(net, kind, &L) ? 0 : L.total_bytes;
}
size_t map_len_of(const mi_nerf_net* net, int kind) {
    HalfLayout L;
    return blob_layout(net, kind, &L) ? 0 : (size_t)L.stream_bytes / 2 + L.side_floats;
}
// step 1: v = stream values | side tables
int blob_values(const mi_nerf_net* net, const mi_nerf_params* p, int kind, const HalfLayout& L, std::vector<float>& v) {
    const size_t n_stream = L.stream_bytes / 2;
    v.reserve(n_stream + L.side_floats);
    if (kind == KIND_F16S_BWD) stream_bwd(net, p, 2, v);
    else stream_fwd(net, p, kind == KIND_BF16 ? 1 : 2, v);
    MN_CHECK_ARG(v.size() == n_stream, "internal: stream of blob kind %d is %zu elements, not %zu", kind, v.size(), n_stream);
    v.resize(n_stream + L.side_floats, 0.0f);
    if (L.side_floats) fill_side(net, p, L, v.data() + n_stream);
    return MI_NERF_OK;
}
int pack_host(const mi_nerf_net* net, const mi_nerf_params* p, int kind, void* blob, size_t blob_bytes) {
    HalfLayout L;
    if (int rc = blob_layout(net, kind, &L)) return rc;
    MN_CHECK_ARG(blob_bytes >= L.total_bytes, "blob too small: %zu < %u", blob_bytes, L.total_bytes);
    if (kind == KIND_F16S) {                                           // refused by name: the caller learns which tensor
        const int D = net->D, W = net->W, in_x = 3 + 6 * net->L_x, in_d = 3 + 6 * net->L_d;
        for (int l = 0; l < D; ++l) {
            const int n_in = l == 0 ? in_x : ((net->skip >= 0 && l == net->skip + 1) ? W + in_x : W);
            if (int rc = check_weights(p->linear_x_w[l], (size_t)W * n_in, "linear_x.weight")) return rc;
        }
        if (int rc = check_weights(p->linear_feat_w, (size_t)W * W, "linear_feat.weight")) return rc;
        if (int rc = check_weights(p->linear_density_w, W, "linear_density.weight")) return rc;
        if (int rc = check_weights(p->linear_d_w, (size_t)(W / 2) * (W + in_d), "linear_d.weight")) return rc;
        if (int rc = check_weights(p->linear_color_w, (size_t)3 * (W / 2), "linear_color.weight")) return rc;
    }
    std::vector<float> v;
    if (int rc = blob_values(net, p, kind, L, v)) return rc;
    const size_t n_stream = L.stream_bytes / 2;
    if (kind == KIND_F16S_BWD)
        for (size_t i = 0; i < n_stream; ++i) MN_CHECK_ARG(fits_f16(v[i]), "a weight (%g) does not fit the f16-split variant", (double)v[i]);
    memset(blob, 0, L.total_bytes);
    fill_header(net, kind, L, (uint32_t*)blob);
    uint16_t* out = (uint16_t*)((char*)blob + L.stream_off);
    for (size_t i = 0; i < n_stream; ++i) out[i] = kind == KIND_BF16 ? f32_to_bf16_rne(v[i]) : split_elem(v[i], i);
    memcpy((char*)blob + L.side_off, v.data() + n_stream, (size_t)L.side_floats * 4);
    return MI_NERF_OK;
}
// gather map over the FLAT parameter vector: one entry per stream ELEMENT, then one per side-table float
int pack_map_host(const mi_nerf_net* net, int kind, int32_t* map, size_t map_len) {
    HalfLayout L;
    if (int rc = blob_layout(net, kind, &L)) return rc;
    const size_t n = (size_t)L.stream_bytes / 2 + L.side_floats;
    MN_CHECK_ARG(map && map_len >= n, "map too small: %zu entries for %zu", map_len, n);
    IndexParams ip;
    if (int rc = make_index_params(net, ip)) return rc;
    std::vector<float> v;
    if (int rc = blob_values(net, &ip.p, kind, L, v)) return rc;
    for (size_t i = 0; i < n; ++i) map[i] = (int32_t)v[i];
    return MI_NERF_OK;
}

}  // namespace

// steps 2 and 3 on the device.  SPLIT: the f16 split instead of bf16 rounding, and stream elements whose weight is NaN or beyond the f16
// range -- the host packer refuses these -- counted into *bad (may be NULL)
template <bool SPLIT>
__global__ __launch_bounds__(256) void pack_apply_half_kernel(const int32_t* __restrict__ map, const float* __restrict__ flat, unsigned n_stream,
                                                               unsigned n_side, unsigned stream_off, unsigned side_off, HeaderWords hdr,
                                                               char* __restrict__ blob, unsigned* __restrict__ bad) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < HEADER_BYTES / 4) ((uint32_t*)blob)[i] = hdr.w[i];
    if (i < n_stream) {
        const int32_t m = map[i];
        if constexpr (SPLIT) {
            const float w = m ? flat[m - 1] : 0.0f;
            if (!(__builtin_fabsf(w) < 65504.0f) && bad) atomicAdd(bad, 1u);
            const _Float16 hi = (_Float16)w;                                          // round to nearest even, like f32_to_f16_rne
            const _Float16 lo = (_Float16)((w - (float)hi) * SPLIT_SCALE);
            ((_Float16*)(blob + stream_off))[i] = (i & 1023u) < 512u ? hi : lo;
        } else {
            unsigned u = m ? __float_as_uint(flat[m - 1]) : 0u;
            u = ((u & 0x7FFFFFFFu) > 0x7F800000u) ? ((u >> 16) | 0x40u) : ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);      // f32_to_bf16_rne
            ((uint16_t*)(blob + stream_off))[i] = (uint16_t)u;
        }
    } else if (i < n_stream + n_side) {
        const int32_t m = map[i];
        ((float*)(blob + side_off))[i - n_stream] = m ? flat[m - 1] : 0.0f;
    }
}

static int pack_apply_half(const mi_nerf_net* net, int kind, const int32_t* map_dev, const float* flat_dev, void* blob_dev, size_t blob_bytes,
                           unsigned* bad_dev, hipStream_t st) {
    HalfLayout L;
    if (int rc = blob_layout(net, kind, &L)) return rc;
    MN_CHECK_ARG(map_dev && flat_dev && blob_dev, "NULL device pointer");
    MN_CHECK_ARG(blob_bytes >= L.total_bytes && ((uintptr_t)blob_dev & 15) == 0, "blob too small (%zu < %u) or not 16-byte aligned", blob_bytes, L.total_bytes);
    HeaderWords h;
    fill_header(net, kind, L, h.w);
    const unsigned n_stream = L.stream_bytes / 2, total = n_stream + L.side_floats;
    const auto kern = kind == KIND_BF16 ? pack_apply_half_kernel<false> : pack_apply_half_kernel<true>;
    hipLaunchKernelGGL(kern, dim3((total + 255) / 256), dim3(256), 0, st, map_dev, flat_dev, n_stream, L.side_floats, L.stream_off, L.side_off, h,
                       (char*)blob_dev, bad_dev);
    MN_LAUNCH_CHECK("pack_apply_half_kernel");
    return MI_NERF_OK;
}

// ---- entry points (half_layout.h) ----------------------------------------------------------------------------------------------------------
size_t packed_bytes_bf16(const mi_nerf_net* net) { return blob_bytes_of(net, KIND_BF16); }
size_t packed_bytes_f16s(const mi_nerf_net* net) { return blob_bytes_of(net, KIND_F16S); }
size_t packed_bytes_bwd_f16s(const mi_nerf_net* net) { return blob_bytes_of(net, KIND_F16S_BWD); }
int pack_bf16(const mi_nerf_net* net, const mi_nerf_params* p, void* blob, size_t n) { return pack_host(net, p, KIND_BF16, blob, n); }
int pack_f16s(const mi_nerf_net* net, const mi_nerf_params* p, void* blob, size_t n) { return pack_host(net, p, KIND_F16S, blob, n); }
int pack_bwd_f16s(const mi_nerf_net* net, const mi_nerf_params* p, void* blob, size_t n) { return pack_host(net, p, KIND_F16S_BWD, blob, n); }
size_t pack_map_bf16_len(const mi_nerf_net* net) { return map_len_of(net, KIND_BF16); }
size_t pack_map_f16s_len(const mi_nerf_net* net) { return map_len_of(net, KIND_F16S); }
size_t pack_map_bwd_f16s_len(const mi_nerf_net* net) { return map_len_of(net, KIND_F16S_BWD); }
int pack_map_bf16(const mi_nerf_net* net, int32_t* map, size_t n) { return pack_map_host(net, KIND_BF16, map, n); }
int pack_map_f16s(const mi_nerf_net* net, int32_t* map, size_t n) { return pack_map_host(net, KIND_F16S, map, n); }
int pack_map_bwd_f16s(const mi_nerf_net* net, int32_t* map, size_t n) { return pack_map_host(net, KIND_F16S_BWD, map, n); }
int pack_apply_bf16(const mi_nerf_net* net, const int32_t* map_dev, const float* flat_dev, void* blob_dev, size_t n, hipStream_t st) {
    return pack_apply_half(net, KIND_BF16, map_dev, flat_dev, blob_dev, n, nullptr, st);
}
int pack_apply_f16s(const mi_nerf_net* net, const int32_t* map_dev, const float* flat_dev, void* blob_dev, size_t n, unsigned* bad_dev, hipStream_t st) {
    return pack_apply_half(net, KIND_F16S, map_dev, flat_dev, blob_dev, n, bad_dev, st);
}
int pack_apply_bwd_f16s(const mi_nerf_net* net, const int32_t* map_dev, const float* flat_dev, void* blob_dev, size_t n, unsigned* bad_dev, hipStream_t st) {
    return pack_apply_half(net, KIND_F16S_BWD, map_dev, flat_dev, blob_dev, n, bad_dev, st);
}

}  // namespace minerf
