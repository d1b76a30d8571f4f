// Helpers shared by the bf16 window-attention kernels (attention_mfma.hip: windows resident in LDS; attention_stream.hip: streaming form for
// 1152-token windows; wmsa_fused.hip: the fused W-MSA forward): head width, log2-domain constants, fragment assembly, the LDS row swizzle and the
// 16-byte head-row store.  Row strides (F_LD, SLD) differ per file and stay there.  Internal linkage (anonymous namespace) in each translation unit.
#pragma once
#include "lds_prims.h"

namespace {

constexpr int HD = 32;
// Scores live in the log2 domain (table column and scale pre-multiplied by log2 e when staged, so the exponential is the bare v_exp_f32); lse is
// stored in the natural-log domain.
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

__device__ __forceinline__ bf16x8 join4(bf16x4 lo, bf16x4 hi) {
    bf16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
}
// A/B fragment whose 8 k-values are contiguous in LDS: row `row`, elements k0..k0+7
__device__ __forceinline__ bf16x8 lds_row8(const bf16* s, int ld, int row, int k0) {
    return *reinterpret_cast<const bf16x8*>(s + row * ld + k0);
}
__device__ __forceinline__ float lds_f32_at(uint32_t addr) { return *reinterpret_cast<lds_f32*>(addr); }
// A lane holds two packed quadruples of one (token, head) row: channels 4g .. 4g+3 (p0) and 16+4g .. 16+4g+3 (p1), g = lane / 16.  Lanes g and
// g ^ 1 swap one of them (ds_bpermute, no memory) so that every lane stores 16 contiguous bytes -- 64 contiguous bytes per row and
// wave-instruction instead of 8-byte pieces.  Every lane of the wave must call (the partner of a valid lane is valid: same row).
__device__ __forceinline__ void store_head_row16(bf16* row_head, int g, uint2 p0, uint2 p1, bool valid) {
    const bool odd = g & 1;
    const uint2 send = odd ? p0 : p1;
    const uint2 got = make_uint2((unsigned)__shfl_xor((int)send.x, 16, 64), (unsigned)__shfl_xor((int)send.y, 16, 64));
    const uint4 out = odd ? make_uint4(got.x, got.y, p1.x, p1.y) : make_uint4(p0.x, p0.y, got.x, got.y);
    if (valid) *reinterpret_cast<uint4*>(row_head + (odd ? 16 + 4 * (g - 1) : 4 * g)) = out;
}
// LDS rows of Q / K / V (/ dO) in attention_mfma.hip and attention_stream.hip: 64 bytes = four 16-byte chunks, UNPADDED, chunk c of row r stored at chunk
// c ^ swz(r) (round 6).  With the 80-byte padded rows of rounds 2-5 the 16-byte row reads were conflict-free but the transposing 8-byte reads of 8
// consecutive rows were 2-way (39 % of the LDS cycles of the 392-token backward were bank conflicts).  swz takes bit 2 of the row into bit 1 of the chunk
// and bit 3 into bit 0: the 16 rows of a row-fragment read (same chunk) land in 16 different 16-byte bank groups, and the 8 rows x 2 chunks of a
// transposing read cover the 64 banks once.  Tile offsets are multiples of 16 rows: a lane's swizzle is a constant of the lane.
__device__ __forceinline__ int swz(int row) { return (((row >> 2) & 1) << 1) | ((row >> 3) & 1); }

}  // namespace
