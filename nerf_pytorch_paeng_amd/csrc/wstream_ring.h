// wstream_ring.h -- what the fragment-file kernel families share, each defined once: the LDS ring that streams the packed weights
// (L2 -> LDS by LDS-DMA) and the 16x16x32 MFMA asm wrappers.  Users: mlp_half_core.h (mlp_bf16.hip, mlp_f16.hip: every <NWV, F16>
// instance) and mlp_f16s_core.h (mlp_f16s.hip, mlp_f16s_stash.hip, dgrad_f16s.hip: the <4, false> instance over a stream of hi / lo
// quads).  The fp32 family's ring (mlp_core.h WRing: 4 slots of 16 KiB, SGPR-base DMAs) has another geometry and is its own type.
#pragma once
#include <type_traits>
#include "half_layout.h"
#include "walk_plan.h"

namespace minerf {

typedef unsigned u32x4b __attribute__((ext_vector_type(4)));

template <int I> using IC = std::integral_constant<int, I>;
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) { f(IC<B>{}); static_for<B + 1, E>(f); }
}

constexpr int HSLOT_QUADS = 32;
constexpr int HSLOT_BYTES = HSLOT_QUADS * QUAD_BYTES;      // 32 KiB
constexpr int HNSLOT = 3;
constexpr int HRING_BYTES = HNSLOT * HSLOT_BYTES;
__host__ __device__ constexpr int hring_dmas(int nwv) { return HSLOT_QUADS / nwv; }      // DMAs per wave per slot (NWV waves per workgroup)

struct HRing {
    const char* sbase;      // stream + wave's 8 KiB share (f16: 16 KiB of the f16s blob's stream)
    unsigned voff;          // lane*16
    unsigned fetch_off, stream_bytes;
    unsigned fetch_lds, lds_lo, lds_hi;
    unsigned read_slot;
    unsigned fetch_src, src_lim;    // f16 only: where this wave's share of the slot being fetched is read (see hring_next_fetch)
};

// ELEMENT TYPE.  Every template below takes `bool F16`: false = a stream of 1 KiB quads read in order (the bf16 stream of mlp_bf16.hip;
// the split-precision kernels' stream of alternating hi and lo quads), true = f16 operands (mlp_f16.hip) read from the split-precision
// blob (mlp_f16s.hip), whose stream is the bf16 stream's quad order with every quad replaced by a (hi, lo) PAIR: the f16 kernel reads the
// hi quads only, so a stream position is 2 KiB of the blob instead of 1 KiB (the same bytes per pass of the ring), and the blob's tail is
// 208 pairs where the bf16 stream has 224 quads -- the 16 quads of padding at the end of the last slot are not in the blob (see
// hring_next_fetch).

// LDS-DMA of the weight stream.  One global_load_lds_dwordx4 moves 64 lanes x 16 B = one 1 KiB quad: global address = per-lane
// VGPR pair + instruction offset, LDS destination = M0 + instruction offset + lane * 16.  M0 is written twice per slot (each
// wave's 8 KiB share = two 4 KiB halves, the 13-bit offset reaches 4 KiB) and is NOT saved / restored around each DMA: nothing
// else in these kernels touches M0 (hipcc uses it only for LDS-direct / GWS / sendmsg / movrel instructions, none of which occur
// here; tests/test_packing_cpu.py disassembles the objects and checks that every M0 write is ours).
__device__ __forceinline__ void set_m0(unsigned lds_in) {
    const unsigned lds_addr = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_in);      // wave-uniform by construction; pin to an SGPR
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(lds_addr) : "memory");
}
template <int IMM>
__device__ __forceinline__ void dma16(const char* gaddr_lane) {
    asm volatile("global_load_lds_dwordx4 %0, off offset:%1" ::"v"(gaddr_lane), "i"(IMM) : "memory");
}
// DMA number i (0 .. HSLOT_QUADS / NWV - 1) of the slot being fetched: a wave's share of a slot is 8 KiB (4 waves per workgroup: two
// 4 KiB halves, M0 set twice) or 4 KiB (8 waves)
// f16: the instruction offset moves the LDS destination by 1 KiB per quad and the global address by the same 1 KiB, so the per-lane
// address carries the other half of the 2 KiB blob stride: quad i of the share is read at 2 KiB * i.  (Mirror: tests/test_f16_mode_cpu.py.)
template <int NWV, bool F16>
__device__ __forceinline__ void hring_dma(const HRing& r, int i) {
    const char* g;
    if constexpr (F16) g = r.sbase + r.fetch_src + r.voff + (i & 3) * 1024 + (i >= 4 ? 8192 : 0);
    else g = r.sbase + r.fetch_off + r.voff + (i >= 4 ? 4096 : 0);
    if (i == 0) set_m0(r.fetch_lds);
    if (i == 4) set_m0(r.fetch_lds + 4096);
    if ((i & 3) == 0) dma16<0>(g);
    else if ((i & 3) == 1) dma16<1024>(g);
    else if ((i & 3) == 2) dma16<2048>(g);
    else dma16<3072>(g);
}
// f16: stream_bytes is the stream as the kernel walks it (body + 224 positions of 2 KiB); the blob ends 16 positions (32 KiB) earlier.  In
// the last slot the shares of waves 2 and 3 are that padding -- never read from LDS -- and re-read the 32 KiB in front of it instead of
// running past the blob (src_lim: the largest fetch_off whose share is inside the blob).
// MIRRORED in numpy by tests/test_f16_mode_cpu.py _ring_reads (with hring_dma's f16 address and the src_lim set-up in hring_start):
// that test checks the f16 addressing against the blobs, so a change to any of the three must be made there too.
template <bool F16>
__device__ __forceinline__ void hring_next_fetch(HRing& r) {
    r.fetch_off += F16 ? 2 * HSLOT_BYTES : HSLOT_BYTES;
    if (r.fetch_off >= r.stream_bytes) r.fetch_off = 0;
    if constexpr (F16) r.fetch_src = r.fetch_off > r.src_lim ? r.fetch_off - HSLOT_BYTES : r.fetch_off;
    r.fetch_lds += HSLOT_BYTES;
    if (r.fetch_lds >= r.lds_hi) r.fetch_lds = r.lds_lo;
}
// consume the next slot: everything but the DMAs issued during the phase that ends here has landed (slot p+1 was
// issued two phases ago); barrier; slot p+2 streams into ring[(p+2)%3] == ring[(p-1)%3] during the new phase.
// Other vector-memory operations of the wave (input prefetches, result stores) share the counter and retire in order:
// they can only make this wait stricter.
template <int NWV, bool F16>
__device__ __forceinline__ void hring_advance(HRing& r) {
    if constexpr (NWV == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    __syncthreads();
    hring_next_fetch<F16>(r);
    r.read_slot = (r.read_slot + 1 == HNSLOT) ? 0 : r.read_slot + 1;
}
// fragment at slot position qs; positions 1 .. HSLOT_QUADS / NWV also issue one of the slot's DMAs (never a burst)
template <int NWV, bool F16>
__device__ __forceinline__ u32x4b hring_read(const char* smem, const HRing& r, int lane, int qs) {
    if (qs >= 1 && qs <= hring_dmas(NWV)) hring_dma<NWV, F16>(r, qs - 1);
    return *(const u32x4b*)(smem + r.read_slot * HSLOT_BYTES + lane * 16 + qs * QUAD_BYTES);
}
// Start-up: a wave's view of the ring at the head of `stream` (smem: the ring's LDS).  The caller then issues slots 0 and 1 in bursts
// (hring_dmas(NWV) x hring_dma, hring_next_fetch, again) and does the first hring_advance, whose barrier also publishes the caller's
// LDS tables; from there on slot p+2 streams in while slot p is consumed.  (The bursts are not in here: with them inside, hipcc
// allocated the registers of every kernel of the family differently -- docs/design/00_round_log.md.)
template <int NWV, bool F16>
__device__ __forceinline__ HRing hring_start(const char* stream, unsigned stream_bytes, const char* smem, unsigned wave, int lane) {
    HRing r;
    r.sbase = stream + wave * (hring_dmas(NWV) * QUAD_BYTES * (F16 ? 2 : 1));
    r.voff = lane * 16;
    r.fetch_off = 0;
    r.stream_bytes = stream_bytes;
    if constexpr (F16) {
        r.fetch_src = 0;
        r.src_lim = stream_bytes - HSLOT_BYTES - (unsigned)(wave + 1) * (hring_dmas(NWV) * 2 * QUAD_BYTES);      // mirror: tests/test_f16_mode_cpu.py
    }
    r.lds_lo = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)smem + wave * (hring_dmas(NWV) * QUAD_BYTES);
    r.lds_hi = r.lds_lo + HRING_BYTES;
    r.fetch_lds = r.lds_lo;
    r.read_slot = HNSLOT - 1;           // the first hring_advance moves to slot 0
    return r;
}

// The 16x16x32 MFMAs as asm statements (hipcc allocates only the VGPR side: THE FRAGMENT FILE, mlp_half_core.h), F16 = the element
// type: acc = A B + c (a job's first MFMA, c = the bias) / acc = A B / acc += A B, each with its B operand from the fragment file
// (IC<R>: a[R:R+3]) or from a VGPR fragment.
template <bool F16, int R>
__device__ __forceinline__ void mfma_first(f32x4& acc, const u32x4b& afrag, IC<R>, const f32x4& c) {
    if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, a[%3:%4], %2" : "=&v"(acc) : "v"(afrag), "v"(c), "n"(R), "n"(R + 3));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, a[%3:%4], %2" : "=&v"(acc) : "v"(afrag), "v"(c), "n"(R), "n"(R + 3));
}
template <bool F16>
__device__ __forceinline__ void mfma_first(f32x4& acc, const u32x4b& afrag, const u32x4b& bfrag, const f32x4& c) {
    if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %3" : "=&v"(acc) : "v"(afrag), "v"(bfrag), "v"(c));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %3" : "=&v"(acc) : "v"(afrag), "v"(bfrag), "v"(c));
}
template <bool F16, int R>
__device__ __forceinline__ void mfma_zero(f32x4& acc, const u32x4b& afrag, IC<R>) {
    if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, a[%2:%3], 0" : "=&v"(acc) : "v"(afrag), "n"(R), "n"(R + 3));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, a[%2:%3], 0" : "=&v"(acc) : "v"(afrag), "n"(R), "n"(R + 3));
}
template <bool F16>
__device__ __forceinline__ void mfma_zero(f32x4& acc, const u32x4b& afrag, const u32x4b& bfrag) {
    if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(afrag), "v"(bfrag));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(afrag), "v"(bfrag));
}
template <bool F16, int R>
__device__ __forceinline__ void mfma_acc(f32x4& acc, const u32x4b& afrag, IC<R>) {
    if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, a[%2:%3], %0" : "+v"(acc) : "v"(afrag), "n"(R), "n"(R + 3));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, a[%2:%3], %0" : "+v"(acc) : "v"(afrag), "n"(R), "n"(R + 3));
}
template <bool F16>
__device__ __forceinline__ void mfma_acc(f32x4& acc, const u32x4b& afrag, const u32x4b& bfrag) {
    if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(afrag), "v"(bfrag));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(afrag), "v"(bfrag));
}

}  // namespace minerf
