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
//     (v_cvt_pk_bf16_f32 + ReLU as v_pk_maximum3_f16 on the packed pair's bit patterns: mlp_half_core.h pack_stage) is dealt out over the groups of job j+1, across
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
// The packers of this stream (host and device) are pack_half.hip's; half_layout.h has the blob layout.
#include "mlp_half_core.h"

namespace minerf {

int mlp_rays_bf16(const mi_nerf_net* net, const void* packed_dev, const float* rays_dev, const float* z_dev, int64_t n_rays, int S,
                  float* raw_dev, hipStream_t st, int points_per_wave, const StratDraw* strat, FineDraw* fine) {
    if (fine) fine->taken = false;
    if (int rc = check_net_half(net, "bf16")) return rc;
    const HalfLayout L = make_half_layout(net->D, net->W, net->skip, HalfStream::QUADS);
    return mlp_rays_half<false>(net, L, packed_dev, rays_dev, z_dev, n_rays, S, raw_dev, st, points_per_wave, strat, fine);
}

}  // namespace minerf
