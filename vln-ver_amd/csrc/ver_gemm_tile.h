// What k_gemm_nn (ver_gemm.hip) and k_wgrad_tn (ver_wgrad.hip) share: the 256 x 256 output tile of 8 waves (2 x 4, wave tile
// 128 x 64), its MFMA shape, the LDS fragment reads, the lattice addressing of the implicit operands, and the host-side
// checks and launch steps of their entry points.  (Not the two reduce kernels of the fp32 partial tiles: one template for
// both compiled to other instructions than k_wgrad_reduce, so each file keeps its own.)
//
// MFMA shape: v_mfma_f32_16x16x32_bf16, one k-step of 32 on 8 x 4 tiles of 16 x 16 per wave (128 accumulator registers).
// The v_mfma_f32_32x32x16_bf16 bodies both kernels were first written on lost two A/B rounds and lie in
// scratch/experiments/k_gemm_nn_mfma32.hip.inc and k_wgrad_tn_mfma32.hip.inc.
#pragma once
#include "ver_common.h"

namespace gemm_tile {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr int kTile = 256;                  // output tile edge

struct Shape {
    typedef f32x4 acc_t;
    static constexpr int NI = 8, NJ = 4, NR = 4, TW = 16;   // MFMA tiles per wave (rows, columns), registers per tile, tile edge
    // accumulator register r of a lane: row reg_row(r) + lane_row(lane) of the MFMA tile, column lane & (TW - 1)
    static __device__ __forceinline__ int reg_row(int r) { return r; }
    static __device__ __forceinline__ int lane_row(int lane) { return 4 * (lane >> 4); }
    // Slab piece (8 rows x 128 B; W of the forward, both operands of the weight gradient): position p of row `row` of row
    // group `rowhalf` (rows 0-7 / 8-15 of the 16-row slab) holds source chunk p ^ swz.  The swizzle is applied to the SOURCE
    // address (the LDS-DMA destination is lane-linear).  Bit 1 of the row moves a row pair 64 B; the two 16-lane groups of a
    // half wave read the SAME 16 columns of rows 0-7 and 8-15 of a slab (k-groups g, g + 1), 4 KiB apart: rows 8-15 swap their
    // 32-byte column pairs, and the half covers all 64 banks -- every transposing read is conflict free.
    static __device__ __forceinline__ int swz(int row, int rowhalf) { return (((row >> 1) & 1) << 2) ^ (rowhalf << 1); }
    // A image of the forward ([256 rows][32 k], 64-byte rows): position p of row `row` holds source chunk p ^ swz_a(row).
    // Lane (i = l & 15, k-group c = l >> 4) reads chunk c of row i.  The 16-lane groups of a ds_read_b128 are lanes {0-3,
    // 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: per row-in-four, a group holds (c, row quarter h = i >> 2) =
    // (0, 0), (0, 3), (1, 1), (1, 2) -- or (1, 0), (1, 3), (0, 1), (0, 2) -- whose positions c ^ f(h) must differ:
    // f = (0, 3, 2, 1) = -h gives {0, 1, 2, 3}
    static __device__ __forceinline__ int swz_a(int row) { return (0 - (row >> 2)) & 3; }
};
static_assert(Shape::NI * Shape::TW == 128 && Shape::NJ * Shape::TW == 64 && Shape::NI * Shape::NJ * Shape::NR == 128,
              "a wave tile is 128 x 64 in 128 accumulator registers");

// LDS reads as inline asm: behind the builtins the compiler waits for vmcnt(0) in front of every LDS read that follows an
// LDS-DMA (it cannot tell the ring slots apart), which would serialise the whole pipeline.  The results are only valid
// behind the s_waitcnt lgkmcnt(0) of the caller's phase() (the compiler does not count these reads).
template <int OFF>
__device__ __forceinline__ i32x2 tr_read(int addr) {
    i32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
template <int OFF>
__device__ __forceinline__ i32x4 row_read(int addr) {
    i32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
// MFMA fragment (8 consecutive k of one column) from the two transposing reads of its k halves
__device__ __forceinline__ bf16x8 frag(i32x2 lo, i32x2 hi) {
    return __builtin_bit_cast(bf16x8, (i32x4)__builtin_shufflevector(lo, hi, 0, 1, 2, 3));
}

// byte offset of the C-vector of cell (b, z = zl + dz, y, x) in a source lattice of layout L (ver_lattice_gather's layouts:
// 0 plain [B,4,H,W,C], 2 z-split [B,2,H,W,2,C], 3 planar z-split [4,B,2,H/2,W/2,2,C]); outside the lattice, or b < 0 (a row
// past M): an offset beyond every buffer range (the DMA then writes zeros).  All lattices here are < 2 GiB (checked by the
// launchers).
constexpr int kOutside = (int)0x80000000;
struct LatticeGeom {
    int B, H, W, C;
};
template <int L>
__device__ __forceinline__ int cell_off(const LatticeGeom& t, int b, int zl, int y, int x, int dz) {
    if ((unsigned)y >= (unsigned)t.H || (unsigned)x >= (unsigned)t.W || b < 0) return kOutside;
    const int j = dz >> 1;                                  // z = zl + dz, dz in {0, 2}: same zl, upper half j
    int v;
    if (L == 0)
        v = ((b * 4 + zl + dz) * t.H + y) * t.W + x;
    else if (L == 2)
        v = ((((b * 2 + zl) * t.H + y) * t.W + x) << 1) + j;
    else
        v = (((((((y & 1) << 1 | (x & 1)) * t.B + b) * 2 + zl) * (t.H >> 1) + (y >> 1)) * (t.W >> 1) + (x >> 1)) << 1) + j;
    return v * t.C * 2;
}

// ---- host side of the entry points (`who`: the entry point's name at the front of a message) ----

// the lattice side of an implicit operand: sizes and layout
inline int check_lattice_args(const char* who, int layout, int B, int H, int W, int C, int N, int nseg) {
    VER_REQUIRE(B >= 0 && H > 0 && W > 0 && C > 0 && N > 0 && nseg > 0, VER_EINVAL, "%s: bad sizes", who);
    VER_REQUIRE(layout == 0 || layout == 2 || layout == 3, VER_EINVAL, "%s: layout %d (0 plain, 2 z-split, 3 planar z-split)", who, layout);
    VER_REQUIRE(layout != 3 || (H % 2 == 0 && W % 2 == 0), VER_EINVAL, "%s: planar needs even H, W", who);
    return VER_OK;
}

// The segments of an implicit operand's K axis, `nseg` triples: (dz in {0, 2}, dy, dx) = the C channels of that neighbouring
// cell, (-1 - block, 0, 0) = the `cw` columns of pattern block `block` of the constant-pattern table (`cst`, `ncst` blocks).
// Checks every triple and returns the width of the K axis in *K.  (`who_tap`: the forward reports a bad tap under the name of
// its oldest entry point.)
inline int check_segments(const char* who, const char* who_tap, const int* taps, int nseg, int C, const void* cst, int ncst, int cw,
                          long* K) {
    long k = 0;
    for (int i = 0; i < nseg; ++i) {
        const int dz = taps[3 * i], dy = taps[3 * i + 1], dx = taps[3 * i + 2];
        if (dz < 0) {
            VER_REQUIRE(cst && -1 - dz < ncst, VER_EINVAL, "%s: segment %d names pattern block %d of %d", who, i, -1 - dz, cst ? ncst : 0);
            k += cw;
        } else {
            VER_REQUIRE((dz == 0 || dz == 2) && dy >= -64 && dy <= 64 && dx >= -64 && dx <= 64, VER_EINVAL,
                        "%s: tap %d = (%d, %d, %d): dz must be 0 or 2", who_tap, i, dz, dy, dx);
            k += C;
        }
    }
    *K = k;
    return VER_OK;
}

// one tile kernel on `blocks` workgroups of 512 threads with `lds_bytes` of dynamic LDS (above the 64 KiB default: the
// attribute first).  The caller picks the instantiation and checks the launch.
template <typename Args>
int launch_tile_kernel(const char* who, void (*kern)(Args), const Args& p, int blocks, int lds_bytes, hipStream_t st) {
    if (int rc = ver_lds_limit(who, (const void*)kern, lds_bytes)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), lds_bytes, st, p);
    return VER_OK;
}
}  // namespace gemm_tile
