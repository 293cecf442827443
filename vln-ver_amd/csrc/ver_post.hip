// Occupancy post-processing on the device (include/ver_ops.h: ver_occ_predict, ver_occ_confusion).
//
// Reference: VoxelFormerOccupancyHead.get_occupancy_prediction, focal-loss branch
// (dense_heads/voxelformer_occupancy_head.py:1505-1540):
//     p = sigmoid(logits [N, C]);  p = cat(p, threshold column);  cls = argmax(p, -1);
//     idx = where(cls < C);  pairs = stack(idx, cls[idx])                  -> int64 [K, 2], ascending voxel index
// As torch ops on the GPU that is five passes and an [N, C+1] temporary; here: one classification pass per row
// (sigmoid in fp32, first-occurrence arg-max exactly as torch.argmax orders ties, NaN counts as the maximum), an
// exclusive scan over 1024-row blocks and one ordered compaction pass.  Integer results: bit-exact by construction
// wherever the fp32 sigmoids of a row are distinct.
// The evaluation metric (ver_occ_confusion: the confusion matrix of SSCMetrics) classifies rows with the same
// row_argmax / threshold_class, so a prediction is the same function in both entry points; the per-element rule and
// threshold_class live in ver_classify.h, which the classifying epilogues of the fused MLP forward share.
#include "ver_classify.h"
#include "ver_common.h"

namespace {
constexpr int kRowsPerBlock = 1024;

// arg-max of the fp32 sigmoids of one row: the class and its probability `pb`
template <bool BF16>
__device__ __forceinline__ int row_argmax(const void* logits, long row, int C, float& pb_out) {
    int best = 0;
    float pb = 0.0f;
    for (int c0 = 0; c0 < C; c0 += 8) {
        float x[8];
        if (BF16) {
            const uint4 t = reinterpret_cast<const uint4*>(logits)[(row * C + c0) / 8];
            const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[2 * j] = __uint_as_float(w[j] << 16);
                x[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
            }
        } else {
            const float4 a = reinterpret_cast<const float4*>(logits)[(row * C + c0) / 4];
            const float4 b = reinterpret_cast<const float4*>(logits)[(row * C + c0) / 4 + 1];
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
            x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = ver_class_prob(x[j]);
            const bool take = (c0 + j == 0) || ver_class_takes(p, pb);
            if (take) {
                best = c0 + j;
                pb = p;
            }
        }
    }
    pb_out = pb;
    return best;
}

template <bool BF16>
__device__ __forceinline__ int classify_row(const void* logits, long row, int C, float thr) {
    float pb;
    const int best = row_argmax<BF16>(logits, row, C, pb);
    return threshold_class(best, pb, thr, C);
}

template <bool BF16>
__global__ __launch_bounds__(256) void k_occ_count(const void* __restrict__ logits, long N, int C, float thr,
                                                   int* __restrict__ block_count) {
    __shared__ int wsum[4];
    const long base = (long)blockIdx.x * kRowsPerBlock;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kRowsPerBlock / 256; ++j) {
        const long row = base + j * 256 + threadIdx.x;
        if (row < N) mine += classify_row<BF16>(logits, row, C, thr) < C ? 1 : 0;
    }
    const unsigned long long b = __ballot(mine & 1), b2 = __ballot(mine & 2), b4 = __ballot(mine & 4);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(b) + 2 * __popcll(b2) + 4 * __popcll(b4);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of the block counts in place (one workgroup); *total = number of occupied rows
__global__ __launch_bounds__(1024) void k_occ_scan(int* __restrict__ block_count, int nblocks, int64_t* __restrict__ total) {
    __shared__ long carry;
    __shared__ int part[1024];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblocks; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        const int v = i < nblocks ? block_count[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {                 // Hillis-Steele inclusive scan
            const int add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        const long c = carry;
        if (i < nblocks) block_count[i] = (int)(c + part[threadIdx.x] - v);
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <bool BF16>
__global__ __launch_bounds__(256) void k_occ_emit(const void* __restrict__ logits, long N, int C, float thr,
                                                  const int* __restrict__ block_off, int64_t* __restrict__ pairs) {
    __shared__ int wsum[4];
    const long base = (long)blockIdx.x * kRowsPerBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    long off = block_off[blockIdx.x];
    for (int j = 0; j < kRowsPerBlock / 256; ++j) {            // slabs of 256 consecutive rows: ascending output order
        const long row = base + j * 256 + threadIdx.x;
        const int cls = row < N ? classify_row<BF16>(logits, row, C, thr) : C;
        const bool occ = cls < C;
        const unsigned long long bal = __ballot(occ);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wsum[w];
            tot += wsum[w];
        }
        if (occ) {
            const long k = off + before + __popcll(bal & below);
            pairs[2 * k] = row;
            pairs[2 * k + 1] = cls;
        }
        off += tot;
        __syncthreads();
    }
}

// ---- confusion matrix (ver_occ_confusion) ------------------------------------------------------------------------------
// One pass over [samples * rows_per_sample, C] logits: every row is classified once (row_argmax), the T thresholds are
// applied to its (best, pb) with threshold_class -- the class classify_row(thr_t) gives -- and the (label, prediction)
// pair is counted in an LDS histogram [T, K, K] of the workgroup; one workgroup covers rows of ONE sample
// (grid = (blocks per sample, samples)) and adds its nonzero bins to hist[sample] with 64-bit global atomics.
// The empty/empty bin holds most voxels: counted in a register per thread and threshold, one LDS add per wave at the end.
constexpr int kConfThreads = 256;
constexpr int kConfUnroll = 4;                        // rows of a thread in flight at once
constexpr int kConfRowsPerThread = 16;
constexpr long kConfRowsPerBlock = (long)kConfThreads * kConfRowsPerThread;
constexpr int kConfMaxT = 8;

struct ConfThresholds {
    float t[kConfMaxT];
};

template <bool BF16>
__global__ __launch_bounds__(kConfThreads) void k_occ_confusion(const void* __restrict__ logits,
                                                                const uint8_t* __restrict__ labels, long rows_per_sample,
                                                                int C, ConfThresholds thr, int T,
                                                                unsigned long long* __restrict__ hist) {
    extern __shared__ int bins[];                     // [T, K, K]
    const int K = C + 1, nbins = T * K * K;
    for (int i = threadIdx.x; i < nbins; i += kConfThreads) bins[i] = 0;
    __syncthreads();
    const long base = (long)blockIdx.y * rows_per_sample;
    const long first = (long)blockIdx.x * kConfRowsPerBlock + threadIdx.x;
    int empty_empty[kConfMaxT];
#pragma unroll
    for (int t = 0; t < kConfMaxT; ++t) empty_empty[t] = 0;
    for (int j = 0; j < kConfRowsPerThread; j += kConfUnroll) {
        int best[kConfUnroll], lab[kConfUnroll];
        float pb[kConfUnroll];
#pragma unroll
        for (int u = 0; u < kConfUnroll; ++u) {
            const long r = first + (long)(j + u) * kConfThreads;
            const bool in = r < rows_per_sample;
            const long row = base + (in ? r : rows_per_sample - 1);     // rows past the end read the last row, count nothing
            const int l = labels[row];
            lab[u] = in ? l : 255;
            best[u] = row_argmax<BF16>(logits, row, C, pb[u]);
        }
#pragma unroll
        for (int u = 0; u < kConfUnroll; ++u) {
            if (lab[u] >= K) continue;                // the reference's `gt < n_cl`: invalid / invisible voxels
#pragma unroll
            for (int t = 0; t < kConfMaxT; ++t) {
                if (t >= T) break;
                const int pred = threshold_class(best[u], pb[u], thr.t[t], C);
                if (lab[u] == C && pred == C) ++empty_empty[t];
                else atomicAdd(&bins[(t * K + lab[u]) * K + pred], 1);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kConfMaxT; ++t) {
        if (t >= T) break;
        int v = empty_empty[t];
        for (int off = VER_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & (VER_WAVE - 1)) == 0 && v) atomicAdd(&bins[(t * K + C) * K + C], v);
    }
    __syncthreads();
    unsigned long long* out = hist + (long)blockIdx.y * nbins;
    for (int i = threadIdx.x; i < nbins; i += kConfThreads) {
        const int v = bins[i];
        if (v) atomicAdd(out + i, (unsigned long long)v);
    }
}
}  // namespace

extern "C" long ver_occ_predict_blocks(long N) { return N <= 0 ? 0 : (N + kRowsPerBlock - 1) / kRowsPerBlock; }

extern "C" int ver_occ_predict(const void* logits, int dtype, long N, int C, float threshold, int32_t* block_work,
                               int64_t* pairs, int64_t* count, void* stream) {
    VER_REQUIRE(N >= 0 && C > 0, VER_EINVAL, "ver_occ_predict: bad shape N=%ld C=%d", N, C);
    VER_REQUIRE(C % 8 == 0, VER_EUNSUPPORTED, "ver_occ_predict: class count %d is not a multiple of 8", C);
    VER_REQUIRE(dtype == VER_F32 || dtype == VER_BF16, VER_EINVAL, "ver_occ_predict: dtype %d", dtype);
    VER_REQUIRE(count, VER_EINVAL, "ver_occ_predict: null count");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), st);
        return e == hipSuccess ? VER_OK : ver_fail(VER_ELAUNCH, "ver_occ_predict: %s", hipGetErrorString(e));
    }
    VER_REQUIRE(logits && block_work && pairs, VER_EINVAL, "ver_occ_predict: null pointer argument");
    VER_REQUIRE(((uintptr_t)logits & 15) == 0, VER_EINVAL, "ver_occ_predict: logits must be 16-byte aligned");
    const long nb = ver_occ_predict_blocks(N);
    VER_REQUIRE(nb < (1L << 31) && N < (1L << 31), VER_EUNSUPPORTED, "ver_occ_predict: more than 2^31 rows");
    if (dtype == VER_BF16) hipLaunchKernelGGL(k_occ_count<true>, dim3((unsigned)nb), dim3(256), 0, st, logits, N, C, threshold, block_work);
    else hipLaunchKernelGGL(k_occ_count<false>, dim3((unsigned)nb), dim3(256), 0, st, logits, N, C, threshold, block_work);
    int rc = ver_check_launch("ver_occ_predict/count");
    if (rc) return rc;
    hipLaunchKernelGGL(k_occ_scan, dim3(1), dim3(1024), 0, st, block_work, (int)nb, count);
    rc = ver_check_launch("ver_occ_predict/scan");
    if (rc) return rc;
    if (dtype == VER_BF16) hipLaunchKernelGGL(k_occ_emit<true>, dim3((unsigned)nb), dim3(256), 0, st, logits, N, C, threshold, block_work, pairs);
    else hipLaunchKernelGGL(k_occ_emit<false>, dim3((unsigned)nb), dim3(256), 0, st, logits, N, C, threshold, block_work, pairs);
    return ver_check_launch("ver_occ_predict/emit");
}

extern "C" int ver_occ_confusion(const void* logits, int dtype, long rows_per_sample, int samples, int C,
                                 const uint8_t* labels, const float* thresholds, int num_thresholds, int64_t* hist,
                                 void* stream) {
    VER_REQUIRE(rows_per_sample >= 0 && samples >= 0, VER_EINVAL, "ver_occ_confusion: bad shape rows_per_sample=%ld samples=%d",
                rows_per_sample, samples);
    VER_REQUIRE(dtype == VER_F32 || dtype == VER_BF16, VER_EINVAL, "ver_occ_confusion: dtype %d", dtype);
    VER_REQUIRE(C >= 8 && C <= 32 && C % 8 == 0, VER_EUNSUPPORTED,
                "ver_occ_confusion: class count %d (built for multiples of 8 in [8, 32])", C);
    VER_REQUIRE(thresholds, VER_EINVAL, "ver_occ_confusion: null thresholds");
    VER_REQUIRE(num_thresholds >= 1 && num_thresholds <= kConfMaxT, VER_EUNSUPPORTED,
                "ver_occ_confusion: %d thresholds (1 to %d)", num_thresholds, kConfMaxT);
    if (rows_per_sample == 0 || samples == 0) return VER_OK;
    VER_REQUIRE(logits && labels && hist, VER_EINVAL, "ver_occ_confusion: null pointer argument");
    VER_REQUIRE(((uintptr_t)logits & 15) == 0, VER_EINVAL, "ver_occ_confusion: logits must be 16-byte aligned");
    VER_REQUIRE(((uintptr_t)hist & 7) == 0, VER_EINVAL, "ver_occ_confusion: hist must be 8-byte aligned");
    const long blocks = (rows_per_sample + kConfRowsPerBlock - 1) / kConfRowsPerBlock;
    // (within these bounds every element index, sample * rows_per_sample * C + ..., is far inside 64 bits)
    VER_REQUIRE(blocks < (1L << 23) && samples < 65536, VER_EUNSUPPORTED,
                "ver_occ_confusion: %ld blocks per sample x %d samples exceed the grid", blocks, samples);
    ConfThresholds thr = {};
    for (int t = 0; t < num_thresholds; ++t) thr.t[t] = thresholds[t];
    const int K = C + 1;
    const size_t lds = (size_t)num_thresholds * K * K * sizeof(int);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, (unsigned)samples);
    if (dtype == VER_BF16)
        hipLaunchKernelGGL(k_occ_confusion<true>, grid, dim3(kConfThreads), lds, st, logits, labels, rows_per_sample, C,
                           thr, num_thresholds, h);
    else
        hipLaunchKernelGGL(k_occ_confusion<false>, grid, dim3(kConfThreads), lds, st, logits, labels, rows_per_sample, C,
                           thr, num_thresholds, h);
    return ver_check_launch("ver_occ_confusion");
}
