// The v_mfma_f32_32x32x16_bf16 body of k_wgrad_tn / k_wgrad_tn_seg (one 16-row slab per k-step, 4 x 2 tiles per wave), out of
// csrc/ver_wgrad.hip at commit 8285707, where `constexpr int kShape = 16` had left it unreachable.  Measured against the shipped
// 16x16x32 body in DESIGN.md 3.3 (table of profiles/gemm_mfma_shape_32_vs_16.jsonl: 2.8 % slower).  Nothing builds it.
// ------------------------------------------------------------------------------------------------------------------
// Fragments of the file, inside its namespace: the shape's constants, read_slab, phase() over KP slabs with the slabs PF
// ahead in flight, the fragment addresses (wgrad_body, SH == 32 branch) and the KP / PF this shape ran with.  wgrad_body,
// phases_from and the kernels carried the template axes <SH, KP, PF>; the accumulators were `f32x16 acc[4][2]`.
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int SH>
struct Shape {
    typedef f32x16 acc_t;
    static constexpr int NI = 4, NJ = 2, NR = 16, TW = 32;
    // accumulator register r of a lane: row reg_row(r) + lane_row(lane) of the tile, column lane & (TW - 1)
    static __device__ __forceinline__ int reg_row(int r) { return (r & 3) + 8 * (r >> 2); }
    static __device__ __forceinline__ int lane_row(int lane) { return 4 * (lane >> 5); }
    // source-side swizzle of a piece (8 rows x 128 B): position p of row `row` of row group `rowhalf` holds chunk p ^ swz
    static __device__ __forceinline__ int swz(int row, int rowhalf) { return ((row >> 1) & 1) << 2; }
};

struct WgradLane {          // per-lane constants of the main loop
    // LDS byte addresses of the fragment reads in ring slot 0 -- 32x32x16: [0], [1] = column tiles 0 / 1 of a 64-column block;
    // 16x16x32: the four 16-column tiles of a block, in the lane's slab of the pair and row half
    int offA[4], offB[4];
    int voA, voG;                       // per-lane source offsets of the two LDS-DMA pieces this wave moves
    int stepA, stepG;                   // bytes per slab of the sources
    int dmaoff;                         // offset of this wave's piece inside the A / G part of a slab
};

// Fragments of ring slot SLOT -> registers (12 transposing reads: A tiles 0..3, G tiles 0..1, lo and hi k halves).
template <int SLOT>
__device__ __forceinline__ void read_slab(const WgradLane& c, i32x2 (&al)[4], i32x2 (&ah)[4], i32x2 (&bl)[2], i32x2 (&bh)[2]) {
    // (the offset field of a DS instruction has 16 bits: slots 4-7 go through base registers 64 KiB up)
    constexpr int SB = (SLOT & 3) * kSlabBytes;
    constexpr int UP = SLOT >= 4 ? 65536 : 0;
    const int a0 = c.offA[0] + UP, a1 = c.offA[1] + UP, b0 = c.offB[0] + UP, b1 = c.offB[1] + UP;
    al[0] = tr_read<SB>(a0);
    ah[0] = tr_read<SB + 512>(a0);
    bl[0] = tr_read<SB>(b0);
    bh[0] = tr_read<SB + 512>(b0);
    al[1] = tr_read<SB>(a1);
    ah[1] = tr_read<SB + 512>(a1);
    bl[1] = tr_read<SB>(b1);
    bh[1] = tr_read<SB + 512>(b1);
    al[2] = tr_read<SB + 1024>(a0);
    ah[2] = tr_read<SB + 1536>(a0);
    al[3] = tr_read<SB + 1024>(a1);
    ah[3] = tr_read<SB + 1536>(a1);
}

// 32x32x16: one phase = KP slabs (ring slots PS*KP ..): fragments -> registers, LDS-DMA of the slabs PF ahead, 8 KP MFMAs.
template <int PS, int KP, int PF, int IMPL>
__device__ __forceinline__ void phase(char* lds, f32x16 (&acc)[4][2], const WgradLane& c, __amdgpu_buffer_rsrc_t ra,
                                      __amdgpu_buffer_rsrc_t rg, unsigned& soA, unsigned& soG, const WgradArgs& t, WTapLane& tl) {
    i32x2 al[KP][4], ah[KP][4], bl[KP][2], bh[KP][2];
    int tnext = 0;
    read_slab<PS * KP>(c, al[0], ah[0], bl[0], bh[0]);
    if constexpr (KP == 2) read_slab<PS * KP + 1>(c, al[KP - 1], ah[KP - 1], bl[KP - 1], bh[KP - 1]);
#pragma unroll
    for (int u = 0; u < KP; ++u) {
        const int ds = (PS * KP + u + PF) % kRing;
        if constexpr (IMPL < 0) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(lds + ds * kSlabBytes + c.dmaoff), 16, c.voA, (int)soA, 0, 0);
        } else {
            static_assert(IMPL < 0 || KP == 1, "implicit A: one slab per phase");
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(lds + ds * kSlabBytes + c.dmaoff), 16, tl.vo, 0, 0, 0);
            tnext = lds_read_b32(tl.taddr);                // the entry of the row after (consumed in this phase's MFMA shadow)
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rg, (lds_void*)(lds + ds * kSlabBytes + kSlabBytes / 2 + c.dmaoff), 16, c.voG, (int)soG, 0, 0);
        soA += (unsigned)c.stepA;
        soG += (unsigned)c.stepG;
    }
    // this wave's pieces of the NEXT phase's slabs have landed (everything younger stays in flight)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (PF - KP)) : "memory");
    __builtin_amdgcn_s_barrier();
    // the fragment halves pass through the wait as operands: whatever the compiler does to them (copies into the
    // MFMA's register tuples) is ordered behind it
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(al[0][0]), "+v"(ah[0][0]), "+v"(al[0][1]), "+v"(ah[0][1]), "+v"(al[0][2]), "+v"(ah[0][2]), "+v"(al[0][3]),
                   "+v"(ah[0][3]), "+v"(bl[0][0]), "+v"(bh[0][0]), "+v"(bl[0][1]), "+v"(bh[0][1]), "+v"(tnext)
                 :
                 : "memory");

    if constexpr (KP == 2)
        asm volatile(""
                     : "+v"(al[KP - 1][0]), "+v"(ah[KP - 1][0]), "+v"(al[KP - 1][1]), "+v"(ah[KP - 1][1]), "+v"(al[KP - 1][2]),
                       "+v"(ah[KP - 1][2]), "+v"(al[KP - 1][3]), "+v"(ah[KP - 1][3]), "+v"(bl[KP - 1][0]), "+v"(bh[KP - 1][0]),
                       "+v"(bl[KP - 1][1]), "+v"(bh[KP - 1][1])
                     :
                     : "memory");
    bf16x8 a[KP][4], b[KP][2];
#pragma unroll
    for (int u = 0; u < KP; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[u][i] = frag(al[u][i], ah[u][i]);
        b[u][0] = frag(bl[u][0], bh[u][0]);
        b[u][1] = frag(bl[u][1], bh[u][1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int u = 0; u < KP; ++u)
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
                acc[it][jt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u][it], b[u][jt], acc[it][jt], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (IMPL >= 0) {
        wtap_step(t, tl, tnext);                            // (a dozen VALU instructions under the MFMAs just issued)
        __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_barrier();
}

// wgrad_body, fragment addresses:
    // transposing fragment reads: 16-lane group q = (k half, column half), lane c of it addresses row c >> 2,
    // columns 4 (c & 3) .. + 3 and receives column c of the group's 4 x 16 block
    if constexpr (SH == 32) {
        const int q = lane >> 4, cl = lane & 15;
        const int lowch = (2 * (q & 1) + ((cl & 3) >> 1)) ^ sh::swz(cl >> 2, q >> 1);
        const int lbase = (int)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
        const int rowoff = lbase + ((q >> 1) * 32 + (cl >> 2)) * 128 + lowch * 16 + (cl & 1) * 8;
        c.offA[0] = rowoff + 2 * wr * 1024;
        c.offA[1] = c.offA[0] ^ 64;
        c.offB[0] = rowoff + wc * 1024 + kSlabBytes / 2;
        c.offB[1] = c.offB[0] ^ 64;
        c.offA[2] = c.offA[3] = c.offB[2] = c.offB[3] = 0;

// slabs per phase and prefetch distance (in slabs) of the product's shape: 16x16x32 a slab pair, requested two phases ahead
// like ver_gemm.hip's; 32x32x16 one slab, three ahead (the best of the distances 3-6 and of the pair forms measured in round 5)
constexpr int kKP = kShape == 16 ? 2 : 1;
constexpr int kPF = kShape == 16 ? 4 : 3;
