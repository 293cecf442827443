// A batch out of a device-resident viewpoint store, by index (include/ver_ops.h: ver_fetch_batch).
//
// Reference: VoxelFormer.get_image_feature (detectors/voxelformer.py:317-325) keeps every feature map it has read in a host
// dict and re-reads occ_gt_path on every step; here the split lives in HBM and a step's batch -- features, cameras, padded
// box tables, sparse occupancy pairs -- is gathered by a device-resident index vector straight into the static buffers of a
// captured step.  Launches on the caller's stream, each only when its group is present:
//   k_fetch_scan    ONE workgroup: the status words, out_counts, and the exclusive scan of the bs fetched pair lengths
//                   (64-bit sums) -> offsets, each clamped to the capacity
//   k_fetch_rows    the feature copy, the only part with volume: a workgroup copies kRowUnits accesses of ONE (sample, camera)
//                   row, with the widest access (16, 8, 4 or 2 bytes) that divides the row bytes and both bases; every lane
//                   issues its loads before its stores.  64-bit element offsets: V * Ncam * row passes 2^31.
//   k_fetch_meta    one workgroup per sample: world2pixel, origin, the leading rows of the box tables
//   k_fetch_pairs   a workgroup covers kPairTile consecutive slots of the OUTPUT pair table below offsets[bs]; a slot finds
//                   its sample by bisection of the offsets and reads its pair at a 64-bit position of the CSR
// A sample whose index is outside [0, V) is an empty sample: zero rows, zero cameras, count 0, no pairs -- nothing is read
// outside the store, and CSR bounds are clamped to [0, pair_total] so that a malformed table cannot point past it either.
// Plain vector stores only, no memset node, no allocation, no host read: the call can be captured.
#include "ver_common.h"

namespace {
constexpr int kThreads = 256;
constexpr int kUnroll = 4;
constexpr int kRowUnits = kThreads * kUnroll;      // accesses of one row a workgroup of k_fetch_rows copies
constexpr int kPairTile = kThreads * kUnroll;      // output pair slots a workgroup of k_fetch_pairs covers
constexpr int kScanThreads = 1024;

__device__ __forceinline__ bool in_store(int v, long V) { return v >= 0 && (long)v < V; }

// [lo, hi) of viewpoint v's pairs in the CSR, clamped into [0, total] and never descending
__device__ __forceinline__ void pair_range(const int64_t* __restrict__ pair_offsets, int v, long total, long& lo, long& hi) {
    lo = pair_offsets[v];
    hi = pair_offsets[v + 1];
    lo = lo < 0 ? 0 : (lo > total ? total : lo);
    hi = hi < lo ? lo : (hi > total ? total : hi);
}

__global__ __launch_bounds__(kScanThreads) void k_fetch_scan(const int32_t* __restrict__ index, int bs, long V,
                                                             const int32_t* __restrict__ count_store,
                                                             int32_t* __restrict__ count_out, int store_cap, int out_cap,
                                                             const int64_t* __restrict__ pair_offsets, long pair_total,
                                                             int32_t* __restrict__ offsets, long capacity,
                                                             int32_t* __restrict__ status) {
    __shared__ long part[kScanThreads];
    __shared__ long carry;
    __shared__ int n_outside, n_cut;
    if (threadIdx.x == 0) {
        carry = 0;
        n_outside = 0;
        n_cut = 0;
    }
    __syncthreads();
    for (int b0 = 0; b0 < bs; b0 += kScanThreads) {
        const int b = b0 + threadIdx.x;
        long len = 0;
        if (b < bs) {
            const int v = index[b];
            const bool ok = in_store(v, V);
            if (!ok) atomicAdd(&n_outside, 1);
            if (count_out) {
                int n = ok ? count_store[v] : 0;
                if (n > out_cap) atomicAdd(&n_cut, 1);
                n = n < 0 ? 0 : n;
                n = n < store_cap ? n : store_cap;
                count_out[b] = n < out_cap ? n : out_cap;
            }
            if (offsets && ok) {
                long lo, hi;
                pair_range(pair_offsets, v, pair_total, lo, hi);
                len = hi - lo;
            }
        }
        part[threadIdx.x] = len;
        __syncthreads();
        for (int d = 1; d < kScanThreads; d <<= 1) {            // Hillis-Steele inclusive scan
            const long add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        const long c = carry;
        if (offsets && b < bs) {
            const long lo = c + part[threadIdx.x] - len;
            offsets[b] = (int32_t)(lo < capacity ? lo : capacity);
        }
        __syncthreads();
        if (threadIdx.x == kScanThreads - 1) carry = c + part[kScanThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long total = carry;
        if (offsets) offsets[bs] = (int32_t)(total < capacity ? total : capacity);
        status[0] = n_outside;
        status[1] = n_cut;
        status[2] = (offsets && total > capacity) ? 1 : 0;
        status[3] = total > 0x7fffffffL ? 0x7fffffff : (int32_t)total;
    }
}

// T: the access (uint4, uint2, uint32_t or uint16_t); `units` accesses per row.  grid = (row chunks, Ncam, bs).
template <typename T>
__global__ __launch_bounds__(kThreads) void k_fetch_rows(const int32_t* __restrict__ index, long V, const T* __restrict__ store,
                                                         T* __restrict__ out, long units) {
    const int cam = blockIdx.y, b = blockIdx.z, ncam = gridDim.y, bs = gridDim.z;
    const int v = index[b];
    const long u0 = (long)blockIdx.x * kRowUnits + threadIdx.x;
    T* __restrict__ dst = out + ((long)cam * bs + b) * units;
    T val[kUnroll];
    if (in_store(v, V)) {
        const T* __restrict__ src = store + ((long)v * ncam + cam) * units;
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
            const long u = u0 + (long)j * kThreads;
            if (u < units) val[j] = src[u];
        }
    } else {
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) val[j] = T{};
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
        const long u = u0 + (long)j * kThreads;
        if (u < units) dst[u] = val[j];
    }
}

// one workgroup per sample: the camera rows and the leading min(count, store_cap, out_cap) rows of the box tables
__global__ __launch_bounds__(kThreads) void k_fetch_meta(const int32_t* __restrict__ index, long V, int ncam,
                                                         const float* __restrict__ w2p_store, const float* __restrict__ origin_store,
                                                         float* __restrict__ w2p_out, float* __restrict__ origin_out,
                                                         const float* __restrict__ box_store, const int64_t* __restrict__ label_store,
                                                         const int32_t* __restrict__ count_store, float* __restrict__ box_out,
                                                         int64_t* __restrict__ label_out, int store_cap, int out_cap, int box_dim) {
    const int b = blockIdx.x;
    const int v = index[b];
    const bool ok = in_store(v, V);
    if (w2p_out) {
        const int n = ncam * 16;
        for (int i = threadIdx.x; i < n; i += kThreads) w2p_out[(long)b * n + i] = ok ? w2p_store[(long)v * n + i] : 0.0f;
        if (threadIdx.x < 3) origin_out[(long)b * 3 + threadIdx.x] = ok ? origin_store[(long)v * 3 + threadIdx.x] : 0.0f;
    }
    if (box_out && ok) {
        int n = count_store[v];
        n = n < 0 ? 0 : n;
        n = n < store_cap ? n : store_cap;
        n = n < out_cap ? n : out_cap;
        const float* __restrict__ src = box_store + (long)v * store_cap * box_dim;
        float* __restrict__ dst = box_out + (long)b * out_cap * box_dim;
        for (int i = threadIdx.x; i < n * box_dim; i += kThreads) dst[i] = src[i];
        for (int i = threadIdx.x; i < n; i += kThreads) label_out[(long)b * out_cap + i] = label_store[(long)v * store_cap + i];
    }
}

__global__ __launch_bounds__(kThreads) void k_fetch_pairs(const int32_t* __restrict__ index, int bs, long V,
                                                          const int2* __restrict__ pair_store,
                                                          const int64_t* __restrict__ pair_offsets, long pair_total,
                                                          const int32_t* __restrict__ offsets, int2* __restrict__ pairs_out) {
    const long live = offsets[bs];
    const long k0 = (long)blockIdx.x * kPairTile + threadIdx.x;
    if ((long)blockIdx.x * kPairTile >= live) return;
    int2 val[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
        const long k = k0 + (long)j * kThreads;
        if (k < live) {
            int lo = 0, hi = bs;                                   // the last b with offsets[b] <= k: offsets[0] = 0 <= k < offsets[bs]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((long)offsets[mid] <= k) lo = mid;
                else hi = mid;
            }
            const int v = index[lo];                               // (a sample with live pairs has an index inside the store)
            long first = 0, last = 0;
            if (in_store(v, V)) pair_range(pair_offsets, v, pair_total, first, last);
            const long at = first + (k - (long)offsets[lo]);
            val[j] = at < last ? pair_store[at] : make_int2(0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
        const long k = k0 + (long)j * kThreads;
        if (k < live) pairs_out[k] = val[j];
    }
}

template <typename T>
int launch_rows(hipStream_t st, const int32_t* index, long V, const void* store, void* out, long row_bytes, int ncam, int bs) {
    const long units = row_bytes / (long)sizeof(T);
    // (units <= row elements < 2^40, so at most 2^30 chunks: the check states the grid's limit where the cast is made)
    const long chunks = (units + kRowUnits - 1) / kRowUnits;
    VER_REQUIRE(chunks <= 0x7fffffffL, VER_EUNSUPPORTED, "ver_fetch_batch: %ld row chunks exceed the grid", chunks);
    const dim3 grid((unsigned)chunks, (unsigned)ncam, (unsigned)bs);
    hipLaunchKernelGGL(k_fetch_rows<T>, grid, dim3(kThreads), 0, st, index, V, (const T*)store, (T*)out, units);
    return ver_check_launch("ver_fetch_batch/rows");
}
}  // namespace

extern "C" long ver_fetch_pair_tile(void) { return kPairTile; }

extern "C" int ver_fetch_batch(const int32_t* index, int bs, long V, int ncam, const void* feat_store, void* feat_out,
                               int feat_dtype, long row, const float* w2p_store, const float* origin_store, float* w2p_out,
                               float* origin_out, const float* box_store, const int64_t* label_store,
                               const int32_t* count_store, float* box_out, int64_t* label_out, int32_t* count_out,
                               int store_cap, int out_cap, int box_dim, const int32_t* pair_store, const int64_t* pair_offsets,
                               long pair_total, int32_t* offsets_out, int32_t* pairs_out, long pair_capacity, int32_t* status,
                               void* stream) {
    VER_REQUIRE(bs >= 0, VER_EINVAL, "ver_fetch_batch: bs=%d", bs);
    if (bs == 0) return VER_OK;
    const bool feats = feat_store || feat_out;
    const bool cams = w2p_store || origin_store || w2p_out || origin_out;
    const bool boxes = box_store || label_store || count_store || box_out || label_out || count_out;
    const bool pairs = pair_store || pair_offsets || offsets_out || pairs_out;
    VER_REQUIRE(V >= 0 && ncam >= 0 && row >= 0 && store_cap >= 0 && out_cap >= 0 && box_dim >= 0 && pair_total >= 0 &&
                    pair_capacity >= 0,
                VER_EINVAL,
                "ver_fetch_batch: negative size V=%ld ncam=%d row=%ld store_cap=%d out_cap=%d box_dim=%d pair_total=%ld "
                "pair_capacity=%ld",
                V, ncam, row, store_cap, out_cap, box_dim, pair_total, pair_capacity);
    VER_REQUIRE(!feats || feat_dtype == VER_F32 || feat_dtype == VER_BF16, VER_EINVAL,
                "ver_fetch_batch: feat_dtype %d (VER_F32 or VER_BF16)", feat_dtype);
    VER_REQUIRE(bs < 65536 && ncam < 65536, VER_EUNSUPPORTED, "ver_fetch_batch: bs=%d ncam=%d exceed the grid (< 65 536 each)", bs, ncam);
    VER_REQUIRE(pair_capacity < (1L << 31), VER_EUNSUPPORTED, "ver_fetch_batch: pair_capacity=%ld exceeds the int32 offsets",
                pair_capacity);
    VER_REQUIRE(index && ((uintptr_t)index & 3) == 0, VER_EINVAL, "ver_fetch_batch: index is null or misaligned");
    VER_REQUIRE(status && ((uintptr_t)status & 3) == 0, VER_EINVAL, "ver_fetch_batch: status is null or misaligned");
    const long esize = feat_dtype == VER_BF16 ? 2 : 4;
    if (feats) {
        VER_REQUIRE(feat_store && feat_out, VER_EINVAL, "ver_fetch_batch: feat_store and feat_out come together (one is null)");
        VER_REQUIRE((((uintptr_t)feat_store | (uintptr_t)feat_out) & (esize - 1)) == 0, VER_EINVAL,
                    "ver_fetch_batch: feat_store / feat_out must be aligned to one element");
        VER_REQUIRE(row < (1L << 40), VER_EUNSUPPORTED, "ver_fetch_batch: row=%ld elements", row);
    }
    if (cams) {
        VER_REQUIRE(w2p_store && origin_store && w2p_out && origin_out, VER_EINVAL,
                    "ver_fetch_batch: w2p_store, origin_store, w2p_out and origin_out come together (one is null)");
        VER_REQUIRE((((uintptr_t)w2p_store | (uintptr_t)origin_store | (uintptr_t)w2p_out | (uintptr_t)origin_out) & 3) == 0,
                    VER_EINVAL, "ver_fetch_batch: a misaligned w2p_store, origin_store, w2p_out or origin_out");
    }
    if (boxes) {
        VER_REQUIRE(count_store && count_out, VER_EINVAL, "ver_fetch_batch: count_store and count_out come with the box group (one is null)");
        VER_REQUIRE((box_store && label_store) || store_cap == 0, VER_EINVAL,
                    "ver_fetch_batch: null box_store or label_store with store_cap=%d", store_cap);
        VER_REQUIRE((box_out && label_out) || out_cap == 0, VER_EINVAL, "ver_fetch_batch: null box_out or label_out with out_cap=%d",
                    out_cap);
        VER_REQUIRE((((uintptr_t)box_store | (uintptr_t)box_out | (uintptr_t)count_store | (uintptr_t)count_out) & 3) == 0 &&
                        (((uintptr_t)label_store | (uintptr_t)label_out) & 7) == 0,
                    VER_EINVAL, "ver_fetch_batch: a misaligned box_store, label_store, count_store, box_out, label_out or count_out");
    }
    if (pairs) {
        VER_REQUIRE(pair_offsets && offsets_out, VER_EINVAL,
                    "ver_fetch_batch: pair_offsets and offsets_out come with the pair group (one is null)");
        VER_REQUIRE(pair_store || pair_total == 0, VER_EINVAL, "ver_fetch_batch: null pair_store with pair_total=%ld", pair_total);
        VER_REQUIRE(pairs_out || pair_capacity == 0, VER_EINVAL, "ver_fetch_batch: null pairs_out with a non-zero pair_capacity");
        VER_REQUIRE((((uintptr_t)pair_store | (uintptr_t)pairs_out | (uintptr_t)pair_offsets) & 7) == 0 &&
                        ((uintptr_t)offsets_out & 3) == 0,
                    VER_EINVAL, "ver_fetch_batch: a misaligned pair_store, pair_offsets, offsets_out or pairs_out (pairs: 8 bytes)");
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_fetch_scan, dim3(1), dim3(kScanThreads), 0, st, index, bs, V, boxes ? count_store : nullptr,
                       boxes ? count_out : nullptr, store_cap, out_cap, pairs ? pair_offsets : nullptr, pair_total,
                       pairs ? offsets_out : nullptr, pair_capacity, status);
    int rc = ver_check_launch("ver_fetch_batch/scan");
    if (rc) return rc;
    if (feats && ncam > 0 && row > 0) {
        const long row_bytes = row * esize;
        const uintptr_t low = (uintptr_t)feat_store | (uintptr_t)feat_out | (uintptr_t)row_bytes;
        if ((low & 15) == 0) rc = launch_rows<uint4>(st, index, V, feat_store, feat_out, row_bytes, ncam, bs);
        else if ((low & 7) == 0) rc = launch_rows<uint2>(st, index, V, feat_store, feat_out, row_bytes, ncam, bs);
        else if ((low & 3) == 0) rc = launch_rows<uint32_t>(st, index, V, feat_store, feat_out, row_bytes, ncam, bs);
        else rc = launch_rows<uint16_t>(st, index, V, feat_store, feat_out, row_bytes, ncam, bs);
        if (rc) return rc;
    }
    const bool tables = boxes && out_cap > 0 && store_cap > 0;
    if (cams || tables) {
        hipLaunchKernelGGL(k_fetch_meta, dim3(bs), dim3(kThreads), 0, st, index, V, ncam, w2p_store, origin_store,
                           cams ? w2p_out : nullptr, origin_out, box_store, label_store, count_store, tables ? box_out : nullptr,
                           label_out, store_cap, out_cap, box_dim);
        rc = ver_check_launch("ver_fetch_batch/meta");
        if (rc) return rc;
    }
    if (pairs && pair_capacity > 0 && pair_total > 0) {
        const unsigned tiles = (unsigned)((pair_capacity + kPairTile - 1) / kPairTile);
        hipLaunchKernelGGL(k_fetch_pairs, dim3(tiles), dim3(kThreads), 0, st, index, bs, V, (const int2*)pair_store, pair_offsets,
                           pair_total, offsets_out, (int2*)pairs_out);
        rc = ver_check_launch("ver_fetch_batch/pairs");
    }
    return rc;
}
