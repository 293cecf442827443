// Occupancy pairs on the device (include/ver_ops.h: ver_occ_pairs): the inverse of ver_occ_targets.
//
// Reference: the tail of VoxelFormerOccupancyHead.get_occupancy_prediction (dense_heads/voxelformer_occupancy_head.py:1535-1540),
//     idx = where(cls < C);  pairs = stack(idx, cls[idx])                  -> int64 [K, 2], ascending voxel index
// on a class map that is already there as bytes (ver_occ_mlp_classes leaves it in the GEMMs' row order).  As torch ops that
// is a permuting copy, a compare, `where` with its host read of K, a gather and a stack; here the bytes of a batch become
// per-sample pairs with offsets in fixed shapes, whatever K is.  Three launches on the caller's stream:
//   k_count    a workgroup counts the occupied voxels among kVoxelsPerBlock consecutive voxels of ONE sample
//              (grid = (blocks per sample, samples)) -> block_work[b * blocks + i]
//   k_scan     one workgroup: exclusive scan of block_work over the whole batch in place (samples are consecutive in the
//              output), then offsets (clamped to the capacity), the true counts and the overflow word
//   k_emit     the same workgroups again: ordered compaction, slab by slab of 256 consecutive voxels; a pair whose slot is at
//              or past the capacity is not written
// A voxel's byte is read where ver_occ_targets writes it (label_index below is its formula): with a row table the reads are
// a gather with stride zdim -- 504 KB per viewpoint, nothing here is bound by bandwidth.  Plain vector stores only.
#include "ver_common.h"

namespace {
constexpr int kThreads = 256;
constexpr int kSlabs = 4;
constexpr int kVoxelsPerBlock = kThreads * kSlabs;

// byte index of voxel v of sample b (ver_targets.hip: label_index), or -1 when a (malformed) row table points outside the buffer
__device__ __forceinline__ long label_index(long v, int b, int bs, long voxel_num, int rows, int zdim,
                                            const int32_t* __restrict__ row_table) {
    if (!row_table) return (long)b * voxel_num + v;
    const int z = (int)(v / rows), q = (int)(v - (long)z * rows);
    const long off = row_table[3 * q], n = row_table[3 * q + 1], loc = row_table[3 * q + 2];
    const long idx = ((long)bs * off + (long)b * n + loc) * zdim + z;
    return (idx >= 0 && idx < (long)bs * voxel_num) ? idx : -1;
}

// the class byte of voxel v of sample b; `classes` (empty) past the sample's end or behind a malformed table entry
__device__ __forceinline__ int voxel_class(const uint8_t* __restrict__ labels, long v, int b, int bs, long voxel_num, int rows,
                                           int zdim, int classes, const int32_t* __restrict__ row_table) {
    if (v >= voxel_num) return classes;
    const long idx = label_index(v, b, bs, voxel_num, rows, zdim, row_table);
    return idx < 0 ? classes : (int)labels[idx];
}

__global__ __launch_bounds__(kThreads) void k_count(const uint8_t* __restrict__ labels, const int32_t* __restrict__ row_table,
                                                    int32_t* __restrict__ block_work, long voxel_num, int rows, int zdim,
                                                    int classes, int bs) {
    __shared__ int wsum[kThreads / VER_WAVE];
    const int b = blockIdx.y;
    const long base = (long)blockIdx.x * kVoxelsPerBlock;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kSlabs; ++j)
        mine += voxel_class(labels, base + j * kThreads + threadIdx.x, b, bs, voxel_num, rows, zdim, classes, row_table) < classes ? 1 : 0;
    for (int off = VER_WAVE / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & (VER_WAVE - 1)) == 0) wsum[threadIdx.x / VER_WAVE] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kThreads / VER_WAVE; ++w) s += wsum[w];
        block_work[(long)b * gridDim.x + blockIdx.x] = s;
    }
}

// Exclusive scan of the block counts of the whole batch in place (one workgroup; the total is below 2^31 because
// bs * voxel_num is), then the per-sample results: sample b starts at the exclusive prefix of its first block.
__global__ __launch_bounds__(1024) void k_scan(int32_t* block_work, int blocks_per_sample, int bs, long capacity,
                                               int32_t* __restrict__ offsets, int32_t* __restrict__ count) {
    __shared__ int carry;
    __shared__ int part[1024];
    const int nblocks = blocks_per_sample * bs;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const int v = i < nblocks ? block_work[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {                 // Hillis-Steele inclusive scan
            const int add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        const int c = carry;
        if (i < nblocks) block_work[i] = c + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + part[1023];
        __syncthreads();
    }
    // (the prefixes were written by this workgroup: the barrier above makes them visible to all of its threads)
    const int total = carry;
    const int cap = capacity < (long)total ? (int)capacity : total;
    for (int b = threadIdx.x; b < bs; b += 1024) {
        const int lo = block_work[(long)b * blocks_per_sample];
        const int hi = b + 1 < bs ? block_work[(long)(b + 1) * blocks_per_sample] : total;
        offsets[b] = lo < cap ? lo : cap;
        count[b] = hi - lo;
    }
    if (threadIdx.x == 0) {
        offsets[bs] = cap;
        count[bs] = total;
        count[bs + 1] = (long)total > capacity ? 1 : 0;
    }
}

template <bool I64>
__global__ __launch_bounds__(kThreads) void k_emit(const uint8_t* __restrict__ labels, const int32_t* __restrict__ row_table,
                                                   const int32_t* __restrict__ block_work, void* __restrict__ pairs,
                                                   long capacity, long voxel_num, int rows, int zdim, int classes, int bs,
                                                   int flat) {
    __shared__ int wsum[kThreads / VER_WAVE];
    const int b = blockIdx.y;
    const long base = (long)blockIdx.x * kVoxelsPerBlock;
    const long shift = flat ? (long)b * voxel_num : 0;
    const int lane = threadIdx.x & (VER_WAVE - 1), wave = threadIdx.x / VER_WAVE;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    long off = block_work[(long)b * gridDim.x + blockIdx.x];
    for (int j = 0; j < kSlabs; ++j) {                         // slabs of 256 consecutive voxels: ascending output order
        const long v = base + j * kThreads + threadIdx.x;
        const int cls = voxel_class(labels, v, b, bs, voxel_num, rows, zdim, classes, row_table);
        const bool occ = cls < classes;
        const unsigned long long bal = __ballot(occ);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kThreads / VER_WAVE; ++w) {
            if (w < wave) before += wsum[w];
            tot += wsum[w];
        }
        const long k = off + before + __popcll(bal & below);
        if (occ && k < capacity) {
            if (I64) reinterpret_cast<longlong2*>(pairs)[k] = make_longlong2(v + shift, cls);
            else reinterpret_cast<int2*>(pairs)[k] = make_int2((int)(v + shift), cls);
        }
        off += tot;
        __syncthreads();
    }
}

long blocks_per_sample(long voxel_num) { return (voxel_num + kVoxelsPerBlock - 1) / kVoxelsPerBlock; }
}  // namespace

extern "C" long ver_occ_pairs_block_size(void) { return kVoxelsPerBlock; }

extern "C" long ver_occ_pairs_blocks(int bs, long voxel_num) {
    return (bs <= 0 || voxel_num <= 0) ? 0 : (long)bs * blocks_per_sample(voxel_num);
}

extern "C" int ver_occ_pairs(const uint8_t* labels, const int32_t* row_table, void* pairs, int pair_dtype, int32_t* offsets,
                             int32_t* count, int32_t* block_work, long capacity, long voxel_num, int zdim, int classes, int bs,
                             int flags, void* stream) {
    VER_REQUIRE(bs >= 0 && voxel_num >= 0 && zdim > 0 && classes >= 1 && capacity >= 0, VER_EINVAL,
                "ver_occ_pairs: bad sizes bs=%d voxel_num=%ld zdim=%d classes=%d capacity=%ld", bs, voxel_num, zdim, classes,
                capacity);
    VER_REQUIRE(pair_dtype == VER_I32 || pair_dtype == VER_I64, VER_EINVAL, "ver_occ_pairs: pair dtype %d (VER_I32 or VER_I64)",
                pair_dtype);
    VER_REQUIRE((flags & ~1) == 0, VER_EINVAL, "ver_occ_pairs: flags=%d (bit 0: flattened-batch voxel indices)", flags);
    if (bs == 0 || voxel_num == 0) return VER_OK;
    VER_REQUIRE(classes < 255, VER_EUNSUPPORTED, "ver_occ_pairs: %d classes (byte labels: 255 marks an invalid voxel)", classes);
    VER_REQUIRE(voxel_num % zdim == 0, VER_EUNSUPPORTED, "ver_occ_pairs: voxel_num %ld is no multiple of zdim %d", voxel_num, zdim);
    VER_REQUIRE(voxel_num < (1L << 31) && (long)bs * voxel_num < (1L << 31), VER_EUNSUPPORTED,
                "ver_occ_pairs: %d x %ld labels do not fit 2^31%s", bs, voxel_num,
                ((flags & 1) && pair_dtype == VER_I32) ? " (nor do flattened-batch indices fit int32 pairs)" : "");
    VER_REQUIRE(bs < 65536 && capacity < (1L << 31), VER_EUNSUPPORTED,
                "ver_occ_pairs: bs=%d capacity=%ld exceed the grid / the int32 offsets", bs, capacity);
    VER_REQUIRE(labels && offsets && count && block_work, VER_EINVAL, "ver_occ_pairs: null pointer argument");
    VER_REQUIRE(pairs || capacity == 0, VER_EINVAL, "ver_occ_pairs: null pairs with a non-zero capacity");
    VER_REQUIRE(((uintptr_t)pairs & (pair_dtype == VER_I64 ? 15 : 7)) == 0, VER_EINVAL,
                "ver_occ_pairs: pairs must be aligned to one (index, class) pair");
    VER_REQUIRE(((uintptr_t)offsets & 3) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)block_work & 3) == 0 &&
                    ((uintptr_t)row_table & 3) == 0,
                VER_EINVAL, "ver_occ_pairs: a misaligned offset, counter, scratch or table pointer");
    hipStream_t st = (hipStream_t)stream;
    const long nb = blocks_per_sample(voxel_num);
    const int rows = (int)(voxel_num / zdim);
    const dim3 grid((unsigned)nb, (unsigned)bs);
    hipLaunchKernelGGL(k_count, grid, dim3(kThreads), 0, st, labels, row_table, block_work, voxel_num, rows, zdim, classes, bs);
    int rc = ver_check_launch("ver_occ_pairs/count");
    if (rc) return rc;
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, block_work, (int)nb, bs, capacity, offsets, count);
    rc = ver_check_launch("ver_occ_pairs/scan");
    if (rc) return rc;
    if (pair_dtype == VER_I64)
        hipLaunchKernelGGL(k_emit<true>, grid, dim3(kThreads), 0, st, labels, row_table, block_work, pairs, capacity, voxel_num,
                           rows, zdim, classes, bs, flags & 1);
    else
        hipLaunchKernelGGL(k_emit<false>, grid, dim3(kThreads), 0, st, labels, row_table, block_work, pairs, capacity, voxel_num,
                           rows, zdim, classes, bs, flags & 1);
    return ver_check_launch("ver_occ_pairs/emit");
}
