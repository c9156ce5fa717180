// mlp_f16.hip -- f16-MFMA variant of the fused positional-encoding + NeRF MLP forward: the bf16 kernel (mlp_bf16.hip, read its header
// first; the code is mlp_half_core.h's, instantiated here with F16 = true) on f16 operands.  Same rate on the matrix pipe, 11 significand
// bits instead of 8: the rounding error of every operand is 8x smaller (2^-12 relative instead of 2^-9).  BASELINE config #5's coarse
// network is the user (MI_NERF_MODE_F16_BF16): bf16 rounding there moves the fine sample positions, because sample_pdf is discontinuous.
//
// What differs from the bf16 instantiation, and nothing else:
//   * v_mfma_f32_16x16x32_f16: the same fragment layouts (16-bit elements, 16x16x32), so the same 256-AGPR fragment file.  It lives in a
//     translation unit of its own: tests/test_packing_cpu.py requires every AGPR-operand MFMA of mlp_bf16.hip's object to be the bf16 one.
//   * WEIGHTS from the split-precision blob (mi_nerf_pack_weights_f16s / mi_nerf_pack_apply_f16s / PackedNeRF.f16s()), hi halves only:
//     that stream is the bf16 stream's quad order with each 1 KiB quad replaced by a (hi, lo) pair, so a stream position is 2 KiB of the
//     blob and the DMA reads every other quad (the same bytes per pass as bf16).  Its tail is 208 pairs where bf16 has 224 quads: the
//     ring walks 224 positions and, in the last slot, re-reads data it never uses instead of running past the blob (hring_next_fetch).
//     No packer of its own: the f16s packers' weight check (|w| < 65 504, not NaN; the device packer's out-of-range count) applies.
//   * ACTIVATIONS packed by v_cvt_pk_f16_f32 (round to nearest even), then v_pk_fma_f16 h * 0 + h -- +-inf (an activation at or beyond
//     65 520) becomes NaN, a finite h stays h -- and the ReLU as v_pk_maximum3_f16, NaN-propagating.  (an integer maximum would turn a
//     NaN with its sign bit set into 0, and a ReLU after an inf would turn -inf into 0.)  So the RANGE CONTRACT of the split-precision mode
//     holds (include/mi_nerf.h): an activation beyond the f16 range gives NaN in every output that depends on it, never a finite value.
//     Two or four packed VALU instructions per tile and pair where bf16 has zero or two.
//   * gamma(x) is evaluated PER CHANNEL (Cody-Waite + Cephes, libm from 2^20 rad on: the split-precision kernel's code), not by angle
//     doubling.  Doubling is up to ~5e-5 off at the top octave: below bf16's half-ulp (~2e-3 at 1.0) by two orders, but a fifth of f16's
//     (2.4e-4 at 1.0), so it would flip the f16 rounding of a share of the top octaves' channels against the oracle's exact sin / cos -- an
//     error of the kernel's own making, on top of the f16 rounding the mode is about.  The cost is 27 more sin / cos per point in the
//     prologue (once per point, on the VALU, not in the MFMA stream).
// Launch structure, shapes (64 / 32 points per wave, chosen per launch), the in-kernel stratified draw of the coarse pass and the fused
// render_rays middle of small coarse launches are the bf16 kernel's (mlp_half_core.h mlp_rays_half).
#include "mlp_half_core.h"

namespace minerf {

// Both layouts share their stream positions, tail body and gamma(x) k-steps by construction (half_layout.h); what is left to hold is the
// ring's side of it: the split-precision tail is half a slot of padding short of the 224 positions the ring walks (hring_next_fetch).
static_assert(TAIL_QUADS - TAIL_PAIRS == HSLOT_QUADS / 2, "the f16 kernel walks the split-precision blob's stream as the bf16 stream");

int mlp_rays_f16(const mi_nerf_net* net, const void* packed_dev, const float* rays_dev, const float* z_dev, int64_t n_rays, int S,
                 float* raw_dev, hipStream_t st, int points_per_wave, const StratDraw* strat, FineDraw* fine) {
    if (fine) fine->taken = false;
    if (int rc = check_net_half(net, "f16")) return rc;
    const HalfLayout L = make_half_layout(net->D, net->W, net->skip, HalfStream::PAIRS);
    return mlp_rays_half<true>(net, L, packed_dev, rays_dev, z_dev, n_rays, S, raw_dev, st, points_per_wave, strat, fine);
}

}  // namespace minerf
