// Forward product of the occupancy head's GEMM layers on gfx950 matrix cores:
//     C[M, N] = A[M, K] * W[K, N] (+ bias[N])        (bf16 operands, fp32 accumulation, bf16 result)
// A = rows of the tap matrix of a lattice layer / of the gathered occ_proj operand (row-major, K contiguous; may be a
// column range of a wider matrix), W = the class weight matrix [K, N] as the layers keep it (row-major, N contiguous):
// dense_heads/upsample.py (_Layer0Z4, _LatticeLayerZ4, _LatticeLayer) and occ_proj_lattice.py, i.e. the reference's three
// ConvTranspose3d and occ_proj (voxelformer_occupancy_head.py:251-258, :560, :571) evaluated on the even lattice.
//
// The kernel is the sibling of k_wgrad_tn (ver_wgrad.hip: same 256 x 256 tile, 8 waves as 2 x 4, two wave groups half a
// phase apart, LDS-DMA ring, counted vmcnt, raw barriers); what differs is the operand with the contraction index on its
// FAST axis:
//   * A tile rows are streamed as [256 rows][32 k] images (64 B per row; a wave instruction moves 16 rows x 64 B), their
//     16-byte chunks XOR-ed on the SOURCE address by a function of the row's quarter of its 16-row tile (Shape::swz_a), and
//     the MFMA fragment of a lane (8 consecutive k of one row) is ONE ds_read_b128, conflict free by that swizzle;
//   * W is streamed in 16-row slabs and read through ds_read_b64_tr_b16 exactly as both operands of k_wgrad_tn;
//   * a phase is 32 of K = ONE k-step of v_mfma_f32_16x16x32_bf16 (8 + 8 fragment reads, 4 LDS-DMA pieces, 32 MFMAs per
//     wave on 8 x 4 tiles; k-groups 0-1 of a lane group come from W slab 0, 2-3 from slab 1), the ring holds four phases
//     (128 KB), pieces are requested two phases ahead;
//   * implicit operand: the stream's place on the K axis (segment, channel offset, segment length, the current buffer
//     resource) is wave-uniform and lives in SGPRs; the K axis is described by one packed 32-bit descriptor per segment in
//     the kernel-argument block, and the descriptor of segment t + 1 is requested by a scalar load when segment t begins, so
//     a segment switch is scalar work + the two lanes' offset arithmetic: the main loop holds no vector-memory instruction
//     but the LDS-DMA pieces and no vmcnt wait but the counted vmcnt(4), and no instantiation has a private segment;
//   * no split over K for the tall products (K = 6 304 .. 38 400 here: 197+ phases per tile; skinny ones -- the 450- and
//     1 800-row operands of a one-viewpoint step, 12-42 tiles -- are cut into K slices with fp32 partial tiles, see
//     ver_gemm_nn_splitk); tiles are dealt to the XCDs in contiguous
//     ranges, the N tiles of one row block next to each other, so that the 32 tiles in flight on an XCD share their A
//     rows and W columns in its L2.
// The MFMA shape, the fragment reads, the swizzles and the lattice addressing are ver_gemm_tile.h's, shared with ver_wgrad.hip.
// (The body this kernel was first written on, two k-steps of the other bf16 MFMA shape per phase, lost both A/B rounds of
// DESIGN.md 3.3 and lies in scratch/experiments/k_gemm_nn_mfma32.hip.inc.)  Implicit and explicit entry points are compared
// bit for bit.
#include "ver_gemm_tile.h"

namespace {
using namespace gemm_tile;
constexpr int kStageBytes = 32768;          // A image [256][32] (16 KB) + two W slabs [16][256] (2 x 8 KB)
constexpr int kStages = 4;
constexpr int kLdsBytes = kStages * kStageBytes;

// Implicit operand (ver_gemm_nn_taps): A is never materialised -- row r of the product is cell (b, zl, y, x) of a Z = 4
// lattice (r = ((b 2 + zl) H + y) W + x), its K axis `ntaps` blocks of C channels, block t = the C-vector of the neighbouring
// cell (zl + dz[t], y + dy[t], x + dx[t]) of the SOURCE lattice (zeros outside): exactly the tap matrix ver_lattice_gather
// writes, read straight from the lattice by the LDS-DMA (a tap block of a row is one contiguous 2 C-byte vector).
struct TapArgs {
    const __bf16* lattice;
    long lattice_bytes;
    int B, H, W, C, ntaps, P;           // H, W: the combined lattice = the rows' grid; P = 2 H W rows per viewpoint
    const float* rowpos;                // [P][N] fp32 or null: added to row r's result by its position r % P
    // constant-pattern segments (descriptor bit 31): CW columns that depend on the row's POSITION r % P only -- a block of
    // cst [P][ncst][CW] bf16 (dense_heads/upsample.py: the 0/1 patterns of the bias-valued odd positions + the 1 column)
    const __bf16* cst;
    long cst_bytes;
    int CW, ncst;
    // one packed descriptor per segment of the K axis (filled by the launcher, read by scalar loads one segment ahead):
    // bits 0-7 dx, 8-15 dy (signed bytes), 16-21 dz in {0, 2} or the pattern block, 22-27 the source plane, bit 31 = pattern
    unsigned desc[64];
    // several source lattices of one shape `plane_elems` elements apart (the four class planes of a layer's output gradient,
    // ver_gemm_nn_segments' d(input) form): a tap reads the plane its descriptor names; lattice_bytes is the size of ONE plane
    long plane_elems;
};

struct GemmArgs {
    const __bf16* A;
    const __bf16* W;
    const float* bias;      // [N] or null
    __bf16* C;
    long lda, ldw, ldc, M;
    int K, N, tiles_n, T, per_xcd;
    int S, Kc;              // split over K (skinny products: a one-viewpoint step has 450 / 1 800 rows, 12-42 tiles):
    float* ws;              //   S slices of Kc columns, fp32 partial tiles [S][M][N], added up by k_gemm_reduce
    TapArgs t;
};

struct GemmLane {
    int offA0;              // A fragment reads (stage 0, row tile 0)
    int offB[4];            // W fragment reads (stage 0): the four 16-column tiles, in the lane's slab and row half
    int voA, voW;           // per-lane source offsets of this wave's LDS-DMA pieces
    int stepW;              // bytes per 16-row slab of W
    int stepA16;            // bytes per 16 rows of A (second LDS-DMA piece of a wave)
    int dmaA, dmaW;         // offsets of this wave's pieces inside a stage
};

struct TapLane {                // implicit operand, per lane (VGPRs): the lane's two rows and their current source offsets
    int b1, zl1, y1, x1, b2, zl2, y2, x2;
    int pos1, pos2;             // r % P of the two rows (constant-pattern segments)
    int vo1, vo2;               // byte offsets of the current segment's vectors (+ this lane's 16-byte chunk)
    int chunk;                  // pch * 16
};
struct TapWave {                // implicit operand, per wave (SGPRs): the DMA stream's place on the K axis
    int tap, ch;                // segment and byte offset inside it of the NEXT piece to request
    int seglen;                 // bytes of the current segment
    unsigned next;              // descriptor of segment tap + 1, loaded when segment tap began
    const __attribute__((address_space(4))) unsigned* tab;     // TapArgs::desc in the kernel-argument block
};

// descriptor `idx` by a scalar load the compiler does not see: the result is valid behind the next s_waitcnt lgkmcnt(0), which
// the caller owes before the first use (desc_ready() / the phase's own wait, which takes ts.next as an operand so that no use
// is scheduled in front of it).  The register must not be copied in between either: when the compiler changes, look at the
// switch path of the main loop in the ISA -- the one-phase-segment cases of tests/test_gemm_tap_stream_gpu.py
// switch in every phase and compare exactly.
__device__ __forceinline__ unsigned desc_load(const TapWave& ts, int idx) {
    unsigned v;
    asm volatile("s_load_dword %0, %1, %2" : "=s"(v) : "s"(ts.tab), "s"(idx * 4) : "memory");
    return v;
}
__device__ __forceinline__ void desc_ready(unsigned& d) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(d) : : "memory"); }

// segment ts.tap begins: its descriptor d -> the lane's two source offsets, the segment's length and the buffer resource its
// pieces go through (the pattern table, or the tap's plane of the lattice).  Everything but o1 / o2 is scalar work.
template <int L>
__device__ __forceinline__ void tap_begin(const TapArgs& t, TapLane& tl, TapWave& ts, unsigned d, __amdgpu_buffer_rsrc_t& ra,
                                          __amdgpu_buffer_rsrc_t rcst) {
    const bool live = ts.tap < t.ntaps;                     // (pieces requested past the last phase: nobody reads them)
    const bool is_cst = live && (d >> 31) != 0;
    const int dx = (int)(d << 24) >> 24, dy = (int)(d << 16) >> 24, dz = (int)(d >> 16) & 63, pl = (int)(d >> 22) & 63;
    int o1 = kOutside, o2 = kOutside, seglen = 2 * t.C;
    if (is_cst) {
        seglen = 2 * t.CW;
        if (tl.b1 >= 0) o1 = (tl.pos1 * t.ncst + dz) * t.CW * 2 + tl.chunk;
        if (tl.b2 >= 0) o2 = (tl.pos2 * t.ncst + dz) * t.CW * 2 + tl.chunk;
        ra = rcst;
    } else if (live) {
        const LatticeGeom geom = {t.B, t.H, t.W, t.C};
        const int c1 = cell_off<L>(geom, tl.b1, tl.zl1, tl.y1 + dy, tl.x1 + dx, dz);
        const int c2 = cell_off<L>(geom, tl.b2, tl.zl2, tl.y2 + dy, tl.x2 + dx, dz);
        if (c1 != kOutside) o1 = c1 + tl.chunk;
        if (c2 != kOutside) o2 = c2 + tl.chunk;
        ra = __builtin_amdgcn_make_buffer_rsrc((void*)(t.lattice + (long)pl * t.plane_elems), 0,
                                               (int)max(0L, min(t.lattice_bytes, 0x7FFFFFFFL)), 0x00020000);
    }
    ts.seglen = seglen;
    tl.vo1 = o1;
    tl.vo2 = o2;
}

// this wave's two A pieces of one phase: explicit operand (IMPL < 0) or straight from the lattice.  PRO: the prologue's two
// requests follow each other without the phase's lgkmcnt(0) in between, so a descriptor loaded by the first is waited for here.
template <int IMPL, bool PRO>
__device__ __forceinline__ void request_a(char* dst, const GemmLane& c, __amdgpu_buffer_rsrc_t& ra, __amdgpu_buffer_rsrc_t rcst,
                                          int& soA, const TapArgs& t, TapLane& tl, TapWave& ts) {
    if constexpr (IMPL < 0) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)dst, 16, c.voA, soA, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(dst + 1024), 16, c.voA, soA + c.stepA16, 0, 0);
        soA += 64;
    } else {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)dst, 16, tl.vo1, ts.ch, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(dst + 1024), 16, tl.vo2, ts.ch, 0, 0);
        ts.ch += 64;
        if (ts.ch == ts.seglen) {                           // next segment: the lane's two source vectors move
            ts.ch = 0;
            ts.tap += 1;
            const unsigned d = ts.next;
            ts.next = desc_load(ts, min(ts.tap + 1, t.ntaps - 1));
            if constexpr (PRO) desc_ready(ts.next);
            tap_begin<IMPL>(t, tl, ts, d, ra, rcst);
        }
    }
}

// one phase = ONE k-step of 32: 8 row reads (the lane's chunk of its row in the eight 16-row tiles), 8 transposing
// reads (4 column tiles, k halves lo / hi of the lane's slab and row group), the LDS-DMA of the phase two ahead, 32 MFMAs.
template <int ST, int IMPL>
__device__ __forceinline__ void phase(char* lds, f32x4 (&acc)[8][4], const GemmLane& c, __amdgpu_buffer_rsrc_t& ra,
                                      __amdgpu_buffer_rsrc_t rw, int& soA, int& soW, const TapArgs& t, TapLane& tl, TapWave& ts,
                                      __amdgpu_buffer_rsrc_t rcst) {
    // (the offset field of a DS instruction has 16 bits: stages 2-3 go through base registers 64 KiB up)
    constexpr int SB = (ST & 1) * kStageBytes;
    constexpr int UP = ST >= 2 ? 65536 : 0;
    const int a0 = c.offA0 + UP;
    i32x4 av[8];
    i32x2 bl[4], bh[4];
    av[0] = row_read<SB>(a0);
    av[1] = row_read<SB + 1024>(a0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = c.offB[q] + UP;
        bl[q] = tr_read<SB + 16384>(b);
        bh[q] = tr_read<SB + 16384 + 512>(b);
        if (q == 0) av[2] = row_read<SB + 2048>(a0), av[3] = row_read<SB + 3072>(a0);
        if (q == 1) av[4] = row_read<SB + 4096>(a0), av[5] = row_read<SB + 5120>(a0);
        if (q == 2) av[6] = row_read<SB + 6144>(a0), av[7] = row_read<SB + 7168>(a0);
    }
    constexpr int DS = ((ST + 2) % kStages) * kStageBytes;
    request_a<IMPL, false>(lds + DS + c.dmaA, c, ra, rcst, soA, t, tl, ts);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void*)(lds + DS + 16384 + c.dmaW), 16, c.voW, soW, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void*)(lds + DS + 24576 + c.dmaW), 16, c.voW, soW + c.stepW, 0, 0);
    soW += 2 * c.stepW;
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // this wave's pieces of the NEXT phase have landed
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3]), "+v"(av[4]), "+v"(av[5]), "+v"(av[6]), "+v"(av[7]), "+v"(bl[0]),
                   "+v"(bh[0]), "+v"(bl[1]), "+v"(bh[1]), "+v"(bl[2]), "+v"(bh[2]), "+v"(bl[3]), "+v"(bh[3])
                 :
                 : "memory");
    if constexpr (IMPL >= 0) asm volatile("" : "+s"(ts.next));      // (a descriptor requested in this phase: valid from here)
    bf16x8 a[8], b[4];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = __builtin_bit_cast(bf16x8, av[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = frag(bl[j], bh[j]);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int it = 0; it < 8; ++it)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[it], b[jt], acc[it][jt], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
}


template <int IMPL>
__global__ __launch_bounds__(512) void k_gemm_nn(GemmArgs p) {
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    // block b runs on XCD b % 8; an XCD works through a contiguous range of tiles (N tiles of a row block adjacent)
    const int item = (int)(blockIdx.x & 7) * p.per_xcd + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= p.per_xcd || item >= p.T * p.S) return;
    const int split = item / p.T, tile = item - split * p.T;
    const int mt = tile / p.tiles_n, nt = tile - mt * p.tiles_n;
    const long row0 = (long)mt * kTile;
    const int k0 = split * p.Kc, klen = min(p.Kc, p.K - k0);
    const int nphase = klen / 32;

    // A: rows row0 .. row0 + 255 (past M: zeros by the buffer range), this slice's columns of the operand -- or the whole
    // source lattice (implicit operand: the per-lane offsets address the tap vectors)
    const __bf16* ab = IMPL < 0 ? p.A + row0 * p.lda + k0 : p.t.lattice;
    const long abytes = IMPL < 0 ? ((p.M - row0 - 1) * p.lda + klen) * 2 : p.t.lattice_bytes;
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)ab, 0, (int)max(0L, min(abytes, 0xFFFFFFFFL)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rcst = __builtin_amdgcn_make_buffer_rsrc((void*)(IMPL < 0 ? ab : p.t.cst), 0,
                                                                          (int)(IMPL < 0 ? 0L : max(0L, min(p.t.cst_bytes, 0x7FFFFFFFL))), 0x00020000);
    // W: columns nt * 256 .., the slice's rows (behind the last element: zeros)
    const __bf16* wb = p.W + (long)k0 * p.ldw + (long)nt * kTile;
    const long wbytes = ((long)(klen - 1) * p.ldw + p.N - (long)nt * kTile) * 2;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)wb, 0, (int)max(0L, min(wbytes, 0xFFFFFFFFL)), 0x00020000);
    GemmLane c;
    {
        // A image piece: 16 rows x 64 B per instruction; lane -> (row l >> 2, position l & 3), position p holds source
        // chunk p ^ Shape::swz_a(row).  This wave moves rows 32 w .. 32 w + 31 (two instructions, + 16 rows = + 1 KiB).
        const int prow = 32 * wave + (lane >> 2);
        const int pch = (lane & 3) ^ Shape::swz_a(prow & 15);
        c.voA = (int)(prow * p.lda * 2) + pch * 16;
        c.dmaA = wave * 2048;
        c.stepA16 = (int)(16 * p.lda * 2);          // (second instruction: rows + 16; same swizzle term)
        // W slab piece: 8 rows x 128 B, chunks XOR-ed by Shape::swz
        const int wrow = lane >> 3, wch = (lane & 7) ^ Shape::swz(wrow, wave >> 2);
        c.voW = (int)(((8 * (wave >> 2) + wrow) * p.ldw + 64 * (wave & 3)) * 2) + wch * 16;
        c.stepW = (int)(16 * p.ldw * 2);
        c.dmaW = wave * 1024;
    }
    // fragment reads.  A (row mode): lane (i = l & 15, k-group g = l >> 4) reads chunk g ^ swz_a(i) of row 128 wr + 16 it + i;
    // W (transposing): group g reads rows 8 (g & 1) .. + 7 of slab g >> 1, lane c of it row c >> 2 (and + 4), chunk
    // 2 q + ((c & 3) >> 1) of column tile q, half c & 1
    {
        const int lbase = (int)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
        const int i = lane & 15, g = lane >> 4;
        c.offA0 = lbase + (128 * wr + i) * 64 + ((g ^ Shape::swz_a(i)) << 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ch = (2 * q + ((i & 3) >> 1)) ^ Shape::swz(i >> 2, g & 1);
            c.offB[q] = lbase + (g >> 1) * 8192 + (g & 1) * 4096 + (i >> 2) * 128 + ch * 16 + (i & 1) * 8 + wc * 1024;
        }
    }
    TapLane tl = {};
    TapWave ts = {};
    if constexpr (IMPL >= 0) {
        // this lane's two rows of the tile -> cells (b, zl, y, x); rows past M: no cell (every tap outside)
        const int prow = 32 * wave + (lane >> 2);
        const int hw = p.t.H * p.t.W;
        auto decode = [&](long r, int& b, int& zl, int& y, int& x) {
            if (r >= p.M) {
                b = -1, zl = y = x = 0;
                return;
            }
            b = (int)(r / p.t.P);
            const int pos = (int)(r - (long)b * p.t.P);
            zl = pos / hw;
            const int rem = pos - zl * hw;
            y = rem / p.t.W;
            x = rem - y * p.t.W;
        };
        decode(row0 + prow, tl.b1, tl.zl1, tl.y1, tl.x1);
        decode(row0 + prow + 16, tl.b2, tl.zl2, tl.y2, tl.x2);
        tl.pos1 = (tl.zl1 * p.t.H + tl.y1) * p.t.W + tl.x1;
        tl.pos2 = (tl.zl2 * p.t.H + tl.y2) * p.t.W + tl.x2;
        tl.chunk = ((lane & 3) ^ Shape::swz_a(prow & 15)) * 16;
        // (the kernel's one parameter starts the kernel-argument block)
        ts.tab = (const __attribute__((address_space(4))) unsigned*)((const __attribute__((address_space(4))) char*)
                     __builtin_amdgcn_kernarg_segment_ptr() + offsetof(GemmArgs, t) + offsetof(TapArgs, desc));
        unsigned d = desc_load(ts, 0);
        desc_ready(d);
        ts.next = desc_load(ts, min(1, p.t.ntaps - 1));
        tap_begin<IMPL>(p.t, tl, ts, d, ra, rcst);
        desc_ready(ts.next);
    }
    Shape::acc_t acc[Shape::NI][Shape::NJ];
#pragma unroll
    for (int it = 0; it < Shape::NI; ++it)
#pragma unroll
        for (int jt = 0; jt < Shape::NJ; ++jt)
#pragma unroll
            for (int r = 0; r < Shape::NR; ++r) acc[it][jt][r] = 0.0f;

    int soA = 0, soW = 0;
    // prologue: phases 0 and 1 in flight, phase 0 landed
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        request_a<IMPL, true>(lds + s * kStageBytes + c.dmaA, c, ra, rcst, soA, p.t, tl, ts);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void*)(lds + s * kStageBytes + 16384 + c.dmaW), 16, c.voW, soW, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void*)(lds + s * kStageBytes + 24576 + c.dmaW), 16, c.voW, soW + c.stepW, 0, 0);
        soW += 2 * c.stepW;
    }
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();          // the second wave group runs half a phase behind

    int s = 0;
    for (; s + kStages <= nphase; s += kStages) {
        phase<0, IMPL>(lds, acc, c, ra, rw, soA, soW, p.t, tl, ts, rcst);
        phase<1, IMPL>(lds, acc, c, ra, rw, soA, soW, p.t, tl, ts, rcst);
        phase<2, IMPL>(lds, acc, c, ra, rw, soA, soW, p.t, tl, ts, rcst);
        phase<3, IMPL>(lds, acc, c, ra, rw, soA, soW, p.t, tl, ts, rcst);
    }
    const int rem = nphase - s;
    if (rem > 0) phase<0, IMPL>(lds, acc, c, ra, rw, soA, soW, p.t, tl, ts, rcst);
    if (rem > 1) phase<1, IMPL>(lds, acc, c, ra, rw, soA, soW, p.t, tl, ts, rcst);
    if (rem > 2) phase<2, IMPL>(lds, acc, c, ra, rw, soA, soW, p.t, tl, ts, rcst);
    if (wr == 0) __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    if (p.S > 1) {
        // partial tile of this K slice -> workspace (fp32, [S][M][N]); bias and rounding happen in k_gemm_reduce
        float* out = p.ws + (long)split * p.M * p.N;
        const long i0 = row0 + 128 * wr + Shape::lane_row(lane);
        const int j0 = nt * kTile + 64 * wc + (lane & (Shape::TW - 1));
#pragma unroll
        for (int it = 0; it < Shape::NI; ++it)
#pragma unroll
            for (int jt = 0; jt < Shape::NJ; ++jt) {
                const int j = j0 + Shape::TW * jt;
#pragma unroll
                for (int r = 0; r < Shape::NR; ++r) {
                    const long i = i0 + Shape::TW * it + Shape::reg_row(r);
                    if (i < p.M && j < p.N) out[i * p.N + j] = acc[it][jt][r];
                }
            }
        return;
    }
    // C tile: register r of tile (it, jt) is row r + 4 (lane >> 4), column lane & 15 of the tile (Shape::reg_row / lane_row).
    // Buffer stores: one 32-bit lane offset + a scalar row offset per store; rows past M fall outside the range and are
    // dropped, columns past N are sent there on purpose.
    __bf16* cb = p.C + row0 * p.ldc + (long)nt * kTile;
    const long cbytes = ((p.M - row0 - 1) * p.ldc + p.N - (long)nt * kTile) * 2;
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)cb, 0, (int)max(0L, min(cbytes, 0xFFFFFFFFL)), 0x00020000);
    const int ldc2 = (int)(p.ldc * 2);
    const int vbase = (128 * wr + Shape::lane_row(lane)) * ldc2 + (64 * wc + (lane & (Shape::TW - 1))) * 2;
    // implicit operand: + rowpos[row % P][j], the position-dependent constant part of the row's result (rows of a tile are
    // consecutive: one conditional subtraction per row instead of a division)
    const bool haspos = IMPL >= 0 && p.t.rowpos != nullptr;
    const int pos0 = haspos ? (int)((row0 + 128 * wr + Shape::lane_row(lane)) % p.t.P) : 0;
#pragma unroll
    for (int jt = 0; jt < Shape::NJ; ++jt) {
        const int j = nt * kTile + 64 * wc + Shape::TW * jt + (lane & (Shape::TW - 1));
        const float bj = (p.bias && j < p.N) ? p.bias[j] : 0.0f;
        const int vo = j < p.N ? vbase + 2 * Shape::TW * jt : -2;
#pragma unroll
        for (int it = 0; it < Shape::NI; ++it) {
            float add[Shape::NR];
#pragma unroll
            for (int r = 0; r < Shape::NR; ++r) {
                add[r] = bj;
                if (haspos) {
                    int pp = pos0 + Shape::TW * it + Shape::reg_row(r);
                    while (pp >= p.t.P) pp -= p.t.P;          // (at most once for P >= 256: the step's lattices have 450+)
                    const long row = row0 + 128 * wr + Shape::lane_row(lane) + Shape::TW * it + Shape::reg_row(r);
                    if (j < p.N && row < p.M) add[r] += p.t.rowpos[(long)pp * p.N + j];
                }
            }
#pragma unroll
            for (int r = 0; r < Shape::NR; ++r) {
                const __bf16 v = (__bf16)(acc[it][jt][r] + add[r]);
                __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(short, v), rc, vo, (Shape::TW * it + Shape::reg_row(r)) * ldc2, 0);
            }
        }
    }
}

// C[i][j] (bf16, row pitch ldc) = sum over the S partial products + bias[j]; 4 columns per thread (N % 4 == 0)
__global__ __launch_bounds__(256) void k_gemm_reduce(const float* __restrict__ ws, const float* __restrict__ bias,
                                                     __bf16* __restrict__ c, long ldc, int S, long M, int N) {
    const long n4 = M * N / 4;
    const long stride = M * N;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n4; e += (long)gridDim.x * 256) {
        float4 acc = *reinterpret_cast<const float4*>(ws + 4 * e);
        for (int s = 1; s < S; ++s) {
            const float4 v = *reinterpret_cast<const float4*>(ws + s * stride + 4 * e);
            acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
        }
        const long i = (4 * e) / N;
        const int j = (int)(4 * e - i * N);
        if (bias) acc.x += bias[j], acc.y += bias[j + 1], acc.z += bias[j + 2], acc.w += bias[j + 3];
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        bf16x4 v;
        v.x = (__bf16)acc.x, v.y = (__bf16)acc.y, v.z = (__bf16)acc.z, v.w = (__bf16)acc.w;
        *reinterpret_cast<bf16x4*>(c + i * ldc + j) = v;
    }
}

// K slices of a skinny product: enough workgroups to fill the chip (>= ~192), slices of at least 512 columns (16 phases: the
// fill / drain of the ring is ~6), whole phases of 32
int pick_k_splits(long M, int K, int N) {
    const long tiles = ((M + kTile - 1) / kTile) * ((N + kTile - 1) / kTile);
    if (tiles >= 96 || K < 2048 || N % 4) return 1;
    int s = (int)((224 + tiles - 1) / tiles);
    if (s > K / 512) s = K / 512;
    if (s > 64) s = 64;
    return s < 2 ? 1 : s;
}
}  // namespace

extern "C" int ver_gemm_nn_splits(long M, int K, int N) {
    if (M <= 0 || K <= 0 || N <= 0) return 1;
    return pick_k_splits(M, K, N);
}

extern "C" int ver_gemm_nn_splitk(const void* a, long lda, const void* w, long ldw, const float* bias, void* c, long ldc, long M,
                                  int K, int N, int splits, void* workspace, long workspace_bytes, void* stream);

extern "C" int ver_gemm_nn(const void* a, long lda, const void* w, long ldw, const float* bias, void* c, long ldc, long M,
                           int K, int N, int flags, void* stream) {
    VER_REQUIRE(flags == 0, VER_EINVAL, "ver_gemm_nn: unknown flags 0x%x", flags);
    return ver_gemm_nn_splitk(a, lda, w, ldw, bias, c, ldc, M, K, N, 1, nullptr, 0, stream);
}

extern "C" int ver_gemm_nn_splitk(const void* a, long lda, const void* w, long ldw, const float* bias, void* c, long ldc, long M,
                                  int K, int N, int splits, void* workspace, long workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    VER_REQUIRE(M >= 0 && K > 0 && N > 0, VER_EINVAL, "ver_gemm_nn: bad sizes M=%ld K=%d N=%d", M, K, N);
    if (M == 0) return VER_OK;
    VER_REQUIRE(a && w && c, VER_EINVAL, "ver_gemm_nn: null pointer argument");
    VER_REQUIRE(splits >= 1 && splits <= 1024, VER_EINVAL, "ver_gemm_nn: %d K slices", splits);
    VER_REQUIRE(splits == 1 || (workspace && workspace_bytes >= (long)splits * M * N * (long)sizeof(float) && N % 4 == 0 && ldc % 4 == 0 &&
                                ((uintptr_t)c & 7) == 0 && ((uintptr_t)workspace & 15) == 0),
                VER_EINVAL, "ver_gemm_nn: %d K slices need an fp32 workspace of %ld bytes, N and ldc multiples of 4", splits,
                (long)splits * M * N * (long)sizeof(float));
    VER_REQUIRE(lda >= K && ldw >= N && ldc >= N, VER_EINVAL, "ver_gemm_nn: row pitch smaller than the row");
    VER_REQUIRE(K % 32 == 0 && K >= 64, VER_EUNSUPPORTED, "ver_gemm_nn: K = %d must be a multiple of 32 (>= 64)", K);
    VER_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)w & 15) == 0, VER_EUNSUPPORTED,
                "ver_gemm_nn: operands must be 16-byte aligned with row pitches that are multiples of 8 elements");
    VER_REQUIRE(256L * lda * 2 + K * 2L < 0x7FFFFFFFL && (long)K * ldw * 2 < 0xFFFFFFFFL && 256L * ldc * 2 < 0x7FFFFFFFL,
                VER_EUNSUPPORTED, "ver_gemm_nn: a tile's operand range exceeds the 32-bit offsets");
    GemmArgs p;
    p.A = (const __bf16*)a;
    p.W = (const __bf16*)w;
    p.bias = bias;
    p.C = (__bf16*)c;
    p.lda = lda;
    p.ldw = ldw;
    p.ldc = ldc;
    p.M = M;
    p.K = K;
    p.N = N;
    p.tiles_n = (N + kTile - 1) / kTile;
    p.T = (int)((M + kTile - 1) / kTile) * p.tiles_n;
    // whole phases per slice; the last slice takes what is left (K % 32 == 0)
    p.Kc = splits == 1 ? K : ((K + splits - 1) / splits + 31) / 32 * 32;
    p.S = splits == 1 ? 1 : (K + p.Kc - 1) / p.Kc;
    p.ws = (float*)workspace;
    p.per_xcd = (p.T * p.S + 7) / 8;
    p.t = TapArgs{};
    if (int rc = launch_tile_kernel("ver_gemm_nn", k_gemm_nn<-1>, p, 8 * p.per_xcd, kLdsBytes, st)) return rc;
    if (p.S > 1) {
        long grid = (M * N / 4 + 255) / 256;
        if (grid > 4096) grid = 4096;
        hipLaunchKernelGGL(k_gemm_reduce, dim3((unsigned)grid), dim3(256), 0, st, (const float*)workspace, bias, (__bf16*)c, ldc, p.S, M, N);
    }
    return ver_check_launch("ver_gemm_nn");
}

extern "C" int ver_gemm_nn_segments(const void* lattice, int layout, int B, int H, int W, int C, const int* taps, int ntaps,
                                    const void* cst, int ncst, int cw, const void* w, long ldw, const float* rowpos,
                                    const float* bias, void* c, long ldc, int N, void* stream);
extern "C" int ver_gemm_nn_planes(const void* lattice, int layout, int B, int H, int W, int C, long plane_elems, int nplanes,
                                  const int* tap_plane, const int* taps, int ntaps, const void* cst, int ncst, int cw,
                                  const void* w, long ldw, const float* rowpos, const float* bias, void* c, long ldc, int N,
                                  void* stream);

extern "C" int ver_gemm_nn_taps(const void* lattice, int layout, int B, int H, int W, int C, const int* taps, int ntaps,
                                const void* w, long ldw, const float* rowpos, const float* bias, void* c, long ldc, int N,
                                void* stream) {
    return ver_gemm_nn_segments(lattice, layout, B, H, W, C, taps, ntaps, nullptr, 0, 0, w, ldw, rowpos, bias, c, ldc, N, stream);
}

extern "C" int ver_gemm_nn_segments(const void* lattice, int layout, int B, int H, int W, int C, const int* taps, int ntaps,
                                    const void* cst, int ncst, int cw, const void* w, long ldw, const float* rowpos,
                                    const float* bias, void* c, long ldc, int N, void* stream) {
    return ver_gemm_nn_planes(lattice, layout, B, H, W, C, 0, 0, nullptr, taps, ntaps, cst, ncst, cw, w, ldw, rowpos, bias, c, ldc, N, stream);
}

extern "C" int ver_gemm_nn_planes(const void* lattice, int layout, int B, int H, int W, int C, long plane_elems, int nplanes,
                                  const int* tap_plane, const int* taps, int ntaps, const void* cst, int ncst, int cw,
                                  const void* w, long ldw, const float* rowpos, const float* bias, void* c, long ldc, int N,
                                  void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = check_lattice_args("ver_gemm_nn_taps", layout, B, H, W, C, N, ntaps)) return rc;
    if (B == 0) return VER_OK;
    VER_REQUIRE(lattice && taps && w && c, VER_EINVAL, "ver_gemm_nn_taps: null pointer argument");
    VER_REQUIRE(ntaps <= 64, VER_EUNSUPPORTED, "ver_gemm_nn_taps: %d taps (at most 64)", ntaps);
    VER_REQUIRE(C % 32 == 0 && C >= 64, VER_EUNSUPPORTED, "ver_gemm_nn_taps: C = %d must be a multiple of 32 (>= 64)", C);
    const long M = (long)B * 2 * H * W, lbytes = (long)B * 4 * H * W * C * 2;
    VER_REQUIRE(cst == nullptr || (ncst > 0 && ncst <= 64 && cw >= 32 && cw % 32 == 0 && ((uintptr_t)cst & 15) == 0), VER_EINVAL,
                "ver_gemm_nn_segments: the constant-pattern table needs 1..64 blocks of a width that is a multiple of 32");
    long K = 0;
    if (int rc = check_segments("ver_gemm_nn_segments", "ver_gemm_nn_taps", taps, ntaps, C, cst, ncst, cw, &K)) return rc;
    VER_REQUIRE(lbytes < 0x7FFFFFFFL, VER_EUNSUPPORTED, "ver_gemm_nn_taps: the source lattice (%ld bytes) exceeds the 2-GiB range of the tap offsets", lbytes);
    VER_REQUIRE(ldw >= N && ldc >= N && ldw % 8 == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)lattice & 15) == 0, VER_EUNSUPPORTED,
                "ver_gemm_nn_taps: w must be 16-byte aligned with a row pitch that is a multiple of 8 elements");
    VER_REQUIRE(K * ldw * 2 < 0xFFFFFFFFL && 256L * ldc * 2 < 0x7FFFFFFFL && K < 0x7FFFFFFFL, VER_EUNSUPPORTED,
                "ver_gemm_nn_taps: a tile's operand range exceeds the 32-bit offsets");
    GemmArgs p;
    p.A = nullptr;
    p.W = (const __bf16*)w;
    p.bias = bias;
    p.C = (__bf16*)c;
    p.lda = 0;
    p.ldw = ldw;
    p.ldc = ldc;
    p.M = M;
    p.K = (int)K;
    p.N = N;
    p.tiles_n = (N + kTile - 1) / kTile;
    p.T = (int)((M + kTile - 1) / kTile) * p.tiles_n;
    p.Kc = (int)K;
    p.S = 1;
    p.ws = nullptr;
    p.per_xcd = (p.T + 7) / 8;
    p.t = TapArgs{};
    p.t.lattice = (const __bf16*)lattice;
    p.t.lattice_bytes = lbytes;
    p.t.B = B, p.t.H = H, p.t.W = W, p.t.C = C, p.t.ntaps = ntaps, p.t.P = 2 * H * W;
    p.t.rowpos = rowpos;
    VER_REQUIRE((plane_elems == 0) == (tap_plane == nullptr) && plane_elems >= 0 && (plane_elems == 0 || (nplanes > 0 && nplanes <= 64 &&
                plane_elems % 8 == 0)), VER_EINVAL, "ver_gemm_nn_planes: plane_elems, nplanes and tap_plane come together");
    p.t.plane_elems = plane_elems;
    p.t.cst = (const __bf16*)cst;
    p.t.cst_bytes = cst ? (long)2 * H * W * ncst * cw * 2 : 0;
    p.t.CW = cw, p.t.ncst = ncst;
    for (int i = 0; i < ntaps; ++i) {
        VER_REQUIRE(!tap_plane || (tap_plane[i] >= 0 && tap_plane[i] < nplanes), VER_EINVAL, "ver_gemm_nn_planes: tap %d reads plane %d of %d", i,
                    tap_plane ? tap_plane[i] : 0, nplanes);
        const int dz = taps[3 * i], dy = taps[3 * i + 1], dx = taps[3 * i + 2];     // (checked by check_segments)
        if (dz < 0)
            p.t.desc[i] = 0x80000000u | (unsigned)(-1 - dz) << 16;
        else
            p.t.desc[i] = (unsigned)(tap_plane ? tap_plane[i] : 0) << 22 | (unsigned)dz << 16 | (unsigned)(dy & 0xFF) << 8 | (unsigned)(dx & 0xFF);
    }
    const auto kern = layout == 0 ? k_gemm_nn<0> : layout == 2 ? k_gemm_nn<2> : k_gemm_nn<3>;
    if (int rc = launch_tile_kernel("ver_gemm_nn_taps", kern, p, 8 * p.per_xcd, kLdsBytes, st)) return rc;
    return ver_check_launch("ver_gemm_nn_taps");
}
