// mlp_f16s.hip -- SPLIT-PRECISION variant of the fused positional-encoding + NeRF MLP forward: fp32-grade results on the f16 matrix pipe.
//
// gfx950 has no reduced-precision fast path for f32 inputs (no xf32): the f32-input MFMA runs at the fp32 vector rate, 1/16 of the
// f16 / bf16 one.  This kernel buys most of that factor back WITHOUT giving up fp32 accuracy: every operand is carried as an f16 pair
//      x = x_hi + x_lo * 2^-11,        x_hi = f16(x),   x_lo = f16((x - x_hi) * 2^11)
// (11 + 11 significand bits; the scale keeps the low part out of the f16 subnormals), and a product W x is three MFMAs
//      acc_hi += W_hi x_hi;      acc_lo += W_hi x_lo;      acc_lo += W_lo x_hi;         y = acc_hi + acc_lo * 2^-11
// with fp32 accumulation -- every f16 x f16 product is exact in fp32, the dropped W_lo x_lo term is 2^-22 of the product.  Measured
// against an fp64 evaluation of the same network the result is as close as the fp32 kernel's (oracle/restate.py mlp_forward_f16split is
// the CPU restatement; tests/test_gpu_parity.py holds the kernel to the fp32 path's own bars).  It is an EXTRA precision mode like the
// bf16 variant, never the headline: bench.py reports it as its own leg against both peaks.
//
// Structure: csrc/mlp_bf16.hip's (read its header first) -- output-tile-major jobs, activations never leave registers, the packed
// accumulators of layer l are the B fragments of layer l+1, the whole AGPR file is a hand-numbered fragment file, weights stream
// L2 -> LDS through a 3 x 32 KiB ring by LDS-DMA, heads on the matrix pipe -- with these differences:
//   * two fragments per operand (hi, lo): the fragment file holds 2 sets x 2 point tiles x 8 fragments x 2 parts x 4 registers = all
//     256 AGPRs, so a wave carries 32 points (2 point tiles of 16), a workgroup 128 per pass of the stream;
//   * the stream holds (hi, lo) quad PAIRS (2.4 MB per network); a group is one k-step = six MFMAs
//         [hi.hi p0] [hi.hi p1] [hi.lo p0] [hi.lo p1] [lo.hi p0] [lo.hi p1]
//     the first two gaps carry the ring work (one A read each, the slot's DMAs), the other four the packing;
//   * packing a pair of accumulator elements (12 VALU): y = fma(lo, 2^-11, hi); Y = fma(hi, 2^11, lo) (= 2^11 y); hi_pk =
//     v_cvt_pk_f16_f32(y0, y1) [v_pk_maximum3_f16 for ReLU, Y = maximum(Y, 0): NaN-propagating]; lo halves by v_fma_mixlo/hi_f16(hi_half, -2^11, Y): the
//     residual (y - hi) 2^11 computed exactly and rounded once; two v_accvgpr_write;
//   * gamma(x) is evaluated in full precision per channel (Cody-Waite + Cephes like the fp32 kernel, libm from 2^20 rad on), not by
//     angle doubling: this variant's contract is fp32-grade output.
// The packers of the (hi, lo) stream (host and device; forward and the backward-data chain) are pack_half.hip's; half_layout.h has the layout.
// Ranges: |weights| and |activations| must stay below the f16 maximum (65 504).  The packer refuses larger weights; an activation beyond it
// comes out as NaN in every output that depends on it, never as a finite value (NaN-propagating ReLU: mlp_f16s_core.h "RANGE CONTRACT").

#include "mlp_f16s_core.h"

namespace minerf {

int mlp_rays_f16s(const mi_nerf_net* net, const void* packed_dev, const float* rays_dev, const float* z_dev, int64_t n_rays, int S,
                  float* raw_dev, hipStream_t st) {
    return launch_f16s<false>(net, packed_dev, rays_dev, z_dev, n_rays, S, raw_dev, nullptr, st);
}
}  // namespace minerf
