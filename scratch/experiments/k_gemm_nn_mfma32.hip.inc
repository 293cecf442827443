// The v_mfma_f32_32x32x16_bf16 body of k_gemm_nn (two k-steps of 4 x 2 tiles per phase), out of csrc/ver_gemm.hip
// at commit 8285707, where `constexpr int kShape = 16` had left it unreachable.  Measured against the shipped 16x16x32 body in
// DESIGN.md 3.3 (tables of profiles/gemm_mfma_shape_32_vs_16.jsonl and profiles/gemm_tap_stream_ab.jsonl).  Nothing builds it.
// ------------------------------------------------------------------------------------------------------------------
// Fragments of the file, inside its namespace: the shape's constants, GemmLane as the body needs it, the fragment addresses
// (k_gemm_nn, kShape == 32 branch), and phase().  The accumulators were `f32x16 acc[4][2]`.
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int SH>
struct Shape {
    typedef f32x16 acc_t;
    static constexpr int NI = 4, NJ = 2, NR = 16, TW = 32;
    // accumulator register r of a lane: row reg_row(r) + lane_row(lane) of the tile, column lane & (TW - 1)
    static __device__ __forceinline__ int reg_row(int r) { return (r & 3) + 8 * (r >> 2); }
    static __device__ __forceinline__ int lane_row(int lane) { return 4 * (lane >> 5); }
    // A image (64-byte rows): position p of row `row` holds source chunk p ^ swz_a(row).  Lane (i = l & 31, k half l >> 5)
    // reads chunk (2 step + (l >> 5)) of row i: every 16-lane group of a ds_read_b128 covers the 16 slots of a bank row
    static __device__ __forceinline__ int swz_a(int row) { return (row >> 2) & 3; }
    // W slab piece (8 rows x 128 B) of row group `rowhalf`: position p of row `row` holds chunk p ^ swz_w (ver_wgrad.hip)
    static __device__ __forceinline__ int swz_w(int row, int rowhalf) { return ((row >> 1) & 1) << 2; }
};

struct GemmLane {
    int offA0, offA1;       // A fragment reads (stage 0, row tile 0): 32x32x16 k-step 0 / 1 of a phase; 16x16x32: offA0 only
    int offB[4];            // W fragment reads (stage 0): 32x32x16 slab 0, column tile 0 / 1; 16x16x32: the four 16-column
                            // tiles, in the lane's slab and row half
    int voA, voW;           // per-lane source offsets of this wave's LDS-DMA pieces
    int stepW;              // bytes per 16-row slab of W
    int stepA16;            // bytes per 16 rows of A (second LDS-DMA piece of a wave)
    int dmaA, dmaW;         // offsets of this wave's pieces inside a stage
};

// k_gemm_nn, fragment addresses:
            const int i = lane & 31;
            c.offA0 = lbase + (128 * wr + i) * 64 + (((lane >> 5) ^ sh::swz_a(i & 15)) << 4);
            c.offA1 = c.offA0 ^ 32;
            const int q = lane >> 4, cl = lane & 15;
            const int lowch = (2 * (q & 1) + ((cl & 3) >> 1)) ^ sh::swz_w(cl >> 2, q >> 1);
            c.offB[0] = lbase + ((q >> 1) * 32 + (cl >> 2)) * 128 + lowch * 16 + (cl & 1) * 8 + wc * 1024;
            c.offB[1] = c.offB[0] ^ 64;
            c.offB[2] = c.offB[3] = 0;

// 32x32x16: one phase = two k-steps of 16 (8 + 8 fragment reads, 16 MFMAs on 4 x 2 tiles)
template <int ST, int IMPL>
__device__ __forceinline__ void phase(char* lds, f32x16 (&acc)[4][2], const GemmLane& c, __amdgpu_buffer_rsrc_t& ra,
                                      __amdgpu_buffer_rsrc_t rw, int& soA, int& soW, const TapArgs& t, TapLane& tl, TapWave& ts,
                                      __amdgpu_buffer_rsrc_t rcst) {
    constexpr int SB = (ST & 1) * kStageBytes;
    constexpr int UP = ST >= 2 ? 65536 : 0;
    const int a0 = c.offA0 + UP, a1 = c.offA1 + UP, b0 = c.offB[0] + UP, b1 = c.offB[1] + UP;
    i32x4 av[2][4];
    i32x2 bl[2][2], bh[2][2];
    // k-step 0: A chunks (l >> 5), W slab 0; k-step 1: A chunks 2 + (l >> 5), W slab 1
    av[0][0] = row_read<SB>(a0);
    av[0][1] = row_read<SB + 2048>(a0);
    bl[0][0] = tr_read<SB + 16384>(b0);
    bh[0][0] = tr_read<SB + 16384 + 512>(b0);
    bl[0][1] = tr_read<SB + 16384>(b1);
    bh[0][1] = tr_read<SB + 16384 + 512>(b1);
    av[0][2] = row_read<SB + 4096>(a0);
    av[0][3] = row_read<SB + 6144>(a0);
    av[1][0] = row_read<SB>(a1);
    av[1][1] = row_read<SB + 2048>(a1);
    bl[1][0] = tr_read<SB + 24576>(b0);
    bh[1][0] = tr_read<SB + 24576 + 512>(b0);
    bl[1][1] = tr_read<SB + 24576>(b1);
    bh[1][1] = tr_read<SB + 24576 + 512>(b1);
    av[1][2] = row_read<SB + 4096>(a1);
    av[1][3] = row_read<SB + 6144>(a1);
    // LDS-DMA of the phase two ahead: this wave's 2 x 16 rows of the A image and its piece of each W slab
    constexpr int DS = ((ST + 2) % kStages) * kStageBytes;
    request_a<IMPL, false>(lds + DS + c.dmaA, c, ra, rcst, soA, t, tl, ts);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void*)(lds + DS + 16384 + c.dmaW), 16, c.voW, soW, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void*)(lds + DS + 24576 + c.dmaW), 16, c.voW, soW + c.stepW, 0, 0);
    soW += 2 * c.stepW;
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");       // this wave's pieces of the NEXT phase have landed
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(av[0][0]), "+v"(av[0][1]), "+v"(av[0][2]), "+v"(av[0][3]), "+v"(av[1][0]), "+v"(av[1][1]), "+v"(av[1][2]),
                   "+v"(av[1][3]), "+v"(bl[0][0]), "+v"(bh[0][0]), "+v"(bl[0][1]), "+v"(bh[0][1]), "+v"(bl[1][0]), "+v"(bh[1][0]),
                   "+v"(bl[1][1]), "+v"(bh[1][1])
                 :
                 : "memory");
    if constexpr (IMPL >= 0) asm volatile("" : "+s"(ts.next));      // (a descriptor requested in this phase: valid from here)
    bf16x8 a[2][4], b[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[u][i] = __builtin_bit_cast(bf16x8, av[u][i]);
        b[u][0] = frag(bl[u][0], bh[u][0]);
        b[u][1] = frag(bl[u][1], bh[u][1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
                acc[it][jt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u][it], b[u][jt], acc[it][jt], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
}
