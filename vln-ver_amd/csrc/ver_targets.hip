// Occupancy targets on the device (include/ver_ops.h: ver_occ_targets).
//
// Reference: the per-sample `gt_occupancy[idx] = cls` of the dataset's sparse (flat voxel index, class) annotation into a
// dense volume filled with `occupancy_classes` (dense_heads/voxelformer_occupancy_head.py:1322-1326, :1404-1408), and the
// label volume of MP3DDataset.evaluate_occ_iou (mp3docc_dataset.py:500-514) with its invalid voxels.  Here the pairs of
// the whole batch arrive as ONE device array and every pair writes ONE byte: at the voxel's place in the reference's
// (Z, X, Y) order, or -- with a row table -- where the group-major row order of the occupancy GEMMs wants it, so that the
// loss kernels read the labels as they are.  Four launches on the caller's stream:
//   k_fill     every byte = `classes` (empty), count and bad = 0
//   k_pairs    one pair per lane: a 32-bit compare-and-swap on the aligned word holding the byte (gfx950 has no byte
//              atomics); among several listings of a voxel the largest class stays.  Counts the empty -> occupied transitions
//   k_verify   every pair reads its voxel back: a class other than its own is a listing that lost (bad[1])
//   k_invalid  invalid voxels = 255, plain byte stores (every writer stores the same value)
// A workgroup handles pairs of ONE sample (grid = (blocks per sample, samples)), so its counts reduce to one atomic per block.
#include "ver_common.h"

namespace {
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_fill(uint32_t* __restrict__ words, long nwords, uint32_t fill,
                                                   int32_t* __restrict__ count, int ncount, int32_t* __restrict__ bad) {
    const long first = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
    const long n4 = (((uintptr_t)words & 15) == 0) ? nwords >> 2 : 0;          // 16-byte stores when aligned for them
    for (long i = first; i < n4; i += step) reinterpret_cast<uint4*>(words)[i] = make_uint4(fill, fill, fill, fill);
    for (long i = (n4 << 2) + first; i < nwords; i += step) words[i] = fill;
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < ncount; i += kThreads) count[i] = 0;
        if (threadIdx.x < 2) bad[threadIdx.x] = 0;
    }
}

template <bool I64>
__device__ __forceinline__ void load_pair(const void* pairs, long i, long& v, long& c) {
    if (I64) {
        const longlong2 t = reinterpret_cast<const longlong2*>(pairs)[i];
        v = t.x;
        c = t.y;
    } else {
        const int2 t = reinterpret_cast<const int2*>(pairs)[i];
        v = t.x;
        c = t.y;
    }
}

// byte index of voxel v of sample b, or -1 when a (malformed) row table points outside the buffer
__device__ __forceinline__ long label_index(long v, int b, int bs, long voxel_num, int rows, int zdim,
                                            const int32_t* __restrict__ row_table) {
    if (!row_table) return (long)b * voxel_num + v;
    const int z = (int)(v / rows), q = (int)(v - (long)z * rows);
    const long off = row_table[3 * q], n = row_table[3 * q + 1], loc = row_table[3 * q + 2];
    const long idx = ((long)bs * off + (long)b * n + loc) * zdim + z;
    return (idx >= 0 && idx < (long)bs * voxel_num) ? idx : -1;
}

// the slice of sample blockIdx.y, clamped into [0, n_total] (offsets are the caller's: never trusted as an index)
__device__ __forceinline__ void sample_slice(const int32_t* __restrict__ offsets, long n_total, long& lo, long& hi) {
    lo = offsets[blockIdx.y];
    hi = offsets[blockIdx.y + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_total ? n_total : hi;
}

// sum of `v` over the workgroup, valid in thread 0
__device__ __forceinline__ int block_sum(int v, int* lds) {
    for (int off = VER_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & (VER_WAVE - 1)) == 0) lds[threadIdx.x / VER_WAVE] = v;
    __syncthreads();
    int s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kThreads / VER_WAVE; ++w) s += lds[w];
    __syncthreads();
    return s;
}

template <bool I64>
__global__ __launch_bounds__(kThreads) void k_pairs(const void* __restrict__ pairs, const int32_t* __restrict__ offsets,
                                                    long n_total, const int32_t* __restrict__ row_table,
                                                    uint32_t* __restrict__ words, int32_t* __restrict__ count,
                                                    int32_t* __restrict__ bad, long voxel_num, int rows, int zdim, int classes,
                                                    int bs) {
    __shared__ int lds[kThreads / VER_WAVE];
    const int b = blockIdx.y;
    long lo, hi;
    sample_slice(offsets, n_total, lo, hi);
    int occupied = 0, rejected = 0;
    for (long i = lo + (long)blockIdx.x * kThreads + threadIdx.x; i < hi; i += (long)gridDim.x * kThreads) {
        long v, c;
        load_pair<I64>(pairs, i, v, c);
        if (v < 0 || v >= voxel_num || c < 0 || c > classes) {
            ++rejected;
            continue;
        }
        if (c == classes) continue;                            // "empty" listed explicitly: the fill already says so
        const long idx = label_index(v, b, bs, voxel_num, rows, zdim, row_table);
        if (idx < 0) {
            ++rejected;
            continue;
        }
        uint32_t* word = words + (idx >> 2);
        const int shift = (int)(idx & 3) * 8;
        const uint32_t e = (uint32_t)classes;
        uint32_t old = e * 0x01010101u;                        // the likely content: if not, the exchange returns the real one
        for (;;) {
            const uint32_t cur = (old >> shift) & 0xffu;
            if (cur != e && cur >= (uint32_t)c) break;         // set already, to this class or a larger one
            const uint32_t want = (old & ~(0xffu << shift)) | ((uint32_t)c << shift);
            if (__hip_atomic_compare_exchange_strong(word, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                occupied += cur == e ? 1 : 0;
                break;
            }
        }
    }
    const int occ = block_sum(occupied, lds), rej = block_sum(rejected, lds);
    if (threadIdx.x == 0) {
        if (occ) {
            __hip_atomic_fetch_add(count + b, occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(count + bs, occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (rej) __hip_atomic_fetch_add(bad, rej, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool I64>
__global__ __launch_bounds__(kThreads) void k_verify(const void* __restrict__ pairs, const int32_t* __restrict__ offsets,
                                                     long n_total, const int32_t* __restrict__ row_table,
                                                     const uint8_t* __restrict__ labels, int32_t* __restrict__ bad,
                                                     long voxel_num, int rows, int zdim, int classes, int bs) {
    __shared__ int lds[kThreads / VER_WAVE];
    long lo, hi;
    sample_slice(offsets, n_total, lo, hi);
    int lost = 0;
    for (long i = lo + (long)blockIdx.x * kThreads + threadIdx.x; i < hi; i += (long)gridDim.x * kThreads) {
        long v, c;
        load_pair<I64>(pairs, i, v, c);
        if (v < 0 || v >= voxel_num || c < 0 || c >= classes) continue;
        const long idx = label_index(v, blockIdx.y, bs, voxel_num, rows, zdim, row_table);
        if (idx >= 0 && labels[idx] != (uint8_t)c) ++lost;
    }
    const int s = block_sum(lost, lds);
    if (threadIdx.x == 0 && s) __hip_atomic_fetch_add(bad + 1, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool I64>
__global__ __launch_bounds__(kThreads) void k_invalid(const void* __restrict__ invalid, const int32_t* __restrict__ offsets,
                                                      long n_total, const int32_t* __restrict__ row_table,
                                                      uint8_t* __restrict__ labels, int32_t* __restrict__ bad, long voxel_num,
                                                      int rows, int zdim, int bs) {
    __shared__ int lds[kThreads / VER_WAVE];
    long lo, hi;
    sample_slice(offsets, n_total, lo, hi);
    int rejected = 0;
    for (long i = lo + (long)blockIdx.x * kThreads + threadIdx.x; i < hi; i += (long)gridDim.x * kThreads) {
        const long v = I64 ? (long)reinterpret_cast<const int64_t*>(invalid)[i] : (long)reinterpret_cast<const int32_t*>(invalid)[i];
        const long idx = (v >= 0 && v < voxel_num) ? label_index(v, blockIdx.y, bs, voxel_num, rows, zdim, row_table) : -1;
        if (idx < 0) ++rejected;
        else labels[idx] = 255;
    }
    const int s = block_sum(rejected, lds);
    if (threadIdx.x == 0 && s) __hip_atomic_fetch_add(bad, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// blocks per sample: about four pairs per lane at an even split, one block at least
unsigned blocks_per_sample(long n_total, int bs) {
    const long b = (n_total / bs + 4 * kThreads - 1) / (4 * kThreads);
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}
}  // namespace

extern "C" int ver_occ_targets(const void* pairs, int pair_dtype, const int32_t* offsets, long n_total, const void* invalid,
                               int invalid_dtype, const int32_t* invalid_offsets, long n_invalid, const int32_t* row_table,
                               uint8_t* labels, int32_t* count, int32_t* bad, long voxel_num, int zdim, int classes, int bs,
                               void* stream) {
    VER_REQUIRE(bs >= 0 && voxel_num >= 0 && zdim > 0 && classes >= 1 && n_total >= 0 && n_invalid >= 0, VER_EINVAL,
                "ver_occ_targets: bad sizes bs=%d voxel_num=%ld zdim=%d classes=%d n_total=%ld n_invalid=%ld", bs, voxel_num,
                zdim, classes, n_total, n_invalid);
    VER_REQUIRE((pair_dtype == VER_I32 || pair_dtype == VER_I64) && (invalid_dtype == VER_I32 || invalid_dtype == VER_I64),
                VER_EINVAL, "ver_occ_targets: index dtypes %d, %d (VER_I32 or VER_I64)", pair_dtype, invalid_dtype);
    if (bs == 0) return VER_OK;
    VER_REQUIRE(classes < 255, VER_EUNSUPPORTED, "ver_occ_targets: %d classes (byte labels: 255 marks an invalid voxel)", classes);
    VER_REQUIRE(voxel_num % zdim == 0, VER_EUNSUPPORTED, "ver_occ_targets: voxel_num %ld is no multiple of zdim %d", voxel_num, zdim);
    VER_REQUIRE(voxel_num < (1L << 31) && (long)bs * voxel_num < (1L << 31), VER_EUNSUPPORTED,
                "ver_occ_targets: %d x %ld labels do not fit 2^31", bs, voxel_num);
    VER_REQUIRE(bs < 65536 && n_total < (1L << 31) && n_invalid < (1L << 31), VER_EUNSUPPORTED,
                "ver_occ_targets: bs=%d n_total=%ld n_invalid=%ld exceed the grid / the int32 offsets", bs, n_total, n_invalid);
    VER_REQUIRE(labels && count && bad && offsets, VER_EINVAL, "ver_occ_targets: null pointer argument");
    VER_REQUIRE((pairs || n_total == 0) && ((invalid && invalid_offsets) || n_invalid == 0), VER_EINVAL,
                "ver_occ_targets: null pointer argument with a non-zero size");
    VER_REQUIRE(((uintptr_t)labels & 3) == 0, VER_EINVAL, "ver_occ_targets: labels must be 4-byte aligned");
    VER_REQUIRE(((uintptr_t)pairs & (pair_dtype == VER_I64 ? 15 : 7)) == 0, VER_EINVAL,
                "ver_occ_targets: pairs must be aligned to one (index, class) pair");
    VER_REQUIRE(((uintptr_t)invalid & (invalid_dtype == VER_I64 ? 7 : 3)) == 0 && ((uintptr_t)offsets & 3) == 0 &&
                    ((uintptr_t)invalid_offsets & 3) == 0 && ((uintptr_t)row_table & 3) == 0 && ((uintptr_t)count & 3) == 0 &&
                    ((uintptr_t)bad & 3) == 0,
                VER_EINVAL, "ver_occ_targets: a misaligned index, offset, table or counter pointer");
    hipStream_t st = (hipStream_t)stream;
    const long total = (long)bs * voxel_num, nwords = (total + 3) >> 2;
    const int rows = (int)(voxel_num / zdim);
    uint32_t* words = reinterpret_cast<uint32_t*>(labels);
    long fb = (nwords / 4 + kThreads - 1) / kThreads;
    fb = fb < 1 ? 1 : (fb > 4096 ? 4096 : fb);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)fb), dim3(kThreads), 0, st, words, nwords, (uint32_t)classes * 0x01010101u, count,
                       bs + 1, bad);
    int rc = ver_check_launch("ver_occ_targets/fill");
    if (rc) return rc;
    if (n_total > 0 && voxel_num > 0) {
        const dim3 grid(blocks_per_sample(n_total, bs), (unsigned)bs);
        if (pair_dtype == VER_I64) {
            hipLaunchKernelGGL(k_pairs<true>, grid, dim3(kThreads), 0, st, pairs, offsets, n_total, row_table, words, count, bad,
                               voxel_num, rows, zdim, classes, bs);
            hipLaunchKernelGGL(k_verify<true>, grid, dim3(kThreads), 0, st, pairs, offsets, n_total, row_table, labels, bad,
                               voxel_num, rows, zdim, classes, bs);
        } else {
            hipLaunchKernelGGL(k_pairs<false>, grid, dim3(kThreads), 0, st, pairs, offsets, n_total, row_table, words, count, bad,
                               voxel_num, rows, zdim, classes, bs);
            hipLaunchKernelGGL(k_verify<false>, grid, dim3(kThreads), 0, st, pairs, offsets, n_total, row_table, labels, bad,
                               voxel_num, rows, zdim, classes, bs);
        }
        rc = ver_check_launch("ver_occ_targets/pairs");
        if (rc) return rc;
    }
    if (n_invalid > 0 && voxel_num > 0) {
        const dim3 grid(blocks_per_sample(n_invalid, bs), (unsigned)bs);
        if (invalid_dtype == VER_I64)
            hipLaunchKernelGGL(k_invalid<true>, grid, dim3(kThreads), 0, st, invalid, invalid_offsets, n_invalid, row_table, labels,
                               bad, voxel_num, rows, zdim, bs);
        else
            hipLaunchKernelGGL(k_invalid<false>, grid, dim3(kThreads), 0, st, invalid, invalid_offsets, n_invalid, row_table, labels,
                               bad, voxel_num, rows, zdim, bs);
        rc = ver_check_launch("ver_occ_targets/invalid");
        if (rc) return rc;
    }
    return VER_OK;
}
