// ver_det_decode: the NMS-free decoding of the detection head's last decoder layer (NMSFreeCoder.decode_padded followed by
// head.get_bboxes_padded; LayoutCoder.decode for the room layout) in one launch -- contract in include/ver_ops.h.
//
// One workgroup per sample.  Every logit becomes a 64-bit key (order word << 32 | flat index): the order word is the usual
// order-preserving transform of the fp32 bits (bf16 widened first), inverted so that an ASCENDING sort of the keys is
// "logit descending, flat index ascending among equal logits"; a NaN gets the largest order word, -0.0 the word of +0.0, and
// the padding up to the next power of two the all-ones key, behind every NaN.  The keys are distinct, so the bitonic network
// (not a stable sort by itself) has exactly one result.  A full sort stayed: at the 16 384-key limit it is 105 passes of 8
// compare-exchanges per thread over 128 KiB of LDS and measures 155 us for 8 samples, at vocc.py's 2 048 keys 23 us (66 passes,
// barrier bound); a radix select of the K-th key would add counting passes of its own before a K-sized sort, for a shape no
// config reaches.
#include <math.h>

#include "ver_common.h"

namespace {

constexpr int kDecodeThreads = 1024;
constexpr int kDecodeMaxSlots = 1024;        // K
constexpr int kDecodeMaxKeys = 16384;        // Q * C: 128 KiB of 8-byte keys

struct CenterRange {
    float v[6];
};

__device__ __forceinline__ uint32_t order_word(float x) {
    if (x != x) return 0xffffffffu;                                      // NaN: after every number
    if (x == 0.0f) return 0x7fffffffu;                                   // -0.0 == +0.0
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? u : ~(u | 0x80000000u);                   // larger logit -> smaller word
}

__device__ __forceinline__ float load_logit(const void* cls, int bf16, size_t at) {
    return bf16 ? bf16_to_f32(static_cast<const uint16_t*>(cls)[at]) : static_cast<const float*>(cls)[at];
}

__global__ __launch_bounds__(kDecodeThreads) void k_det_decode(const void* __restrict__ cls, int bf16,
                                                               const float* __restrict__ box, int box_ld,
                                                               float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                               int* __restrict__ out_labels, uint8_t* __restrict__ out_valid,
                                                               int* __restrict__ out_query, CenterRange rng, float threshold,
                                                               int flags, int Q, int C, int K, int codes, int n) {
    extern __shared__ unsigned long long decode_keys[];                  // [n], n = the power of two >= Q * C
    const int tid = threadIdx.x, threads = blockDim.x;
    const size_t b = blockIdx.x;
    const int qc = Q * C;
    if (cls != nullptr) {
        for (int i = tid; i < n; i += threads) {
            decode_keys[i] = i < qc ? ((unsigned long long)order_word(load_logit(cls, bf16, b * qc + i)) << 32) | (unsigned)i
                                    : ~0ULL;
        }
        __syncthreads();
        for (int k = 2; k <= n; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (n >> 1); t += threads) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const unsigned long long a = decode_keys[lo], c = decode_keys[hi];
                    if ((a > c) == ((lo & k) == 0)) {
                        decode_keys[lo] = c;
                        decode_keys[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
    }
    const int out_ld = codes - 1;
    for (int slot = tid; slot < K; slot += threads) {
        int q = slot, label = 0;
        float logit = 0.0f, score = 0.0f;
        if (cls != nullptr) {
            const int idx = (int)(decode_keys[slot] & 0xffffffffULL);    // < Q * C: K <= Q * C and the padding sorts last
            q = idx / C;
            label = idx - q * C;
            logit = load_logit(cls, bf16, b * qc + idx);
            score = 1.0f / (1.0f + expf(-logit));
        }
        const float* row = box + (b * Q + q) * (size_t)box_ld;
        const float cx = row[0], cy = row[1], cz = row[4];
        const float w = expf(row[2]), l = expf(row[3]), h = expf(row[5]);
        const float yaw = atan2f(row[6], row[7]);
        bool ok = cx >= rng.v[0] && cx <= rng.v[3] && cy >= rng.v[1] && cy <= rng.v[4] && cz >= rng.v[2] && cz <= rng.v[5];
        if (flags & 2) ok = ok && score > threshold;
        ok = ok && logit == logit;
        const size_t at = b * K + slot;
        float* o = out_boxes + at * out_ld;
        o[0] = cx;
        o[1] = cy;
        o[2] = (flags & 1) ? cz - 0.5f * h : cz;
        o[3] = w;
        o[4] = l;
        o[5] = h;
        o[6] = yaw;
        if (codes == 10) {
            o[7] = row[8];
            o[8] = row[9];
        }
        out_scores[at] = score;
        out_labels[at] = label;
        out_valid[at] = ok ? 1 : 0;
        if (out_query != nullptr) out_query[at] = q;
    }
}

}  // namespace

extern "C" int ver_det_decode(const void* cls, int cls_dtype, const float* box, int box_ld, float* out_boxes,
                              float* out_scores, int32_t* out_labels, uint8_t* out_valid, int32_t* out_query,
                              const float* center_range, float score_threshold, int flags, int B, int Q, int C, int K,
                              int codes, void* stream) {
    VER_REQUIRE(B >= 0 && Q >= 1 && (cls == nullptr || C >= 1) && K >= 0, VER_EINVAL,
                "ver_det_decode: bad sizes B=%d Q=%d C=%d K=%d", B, Q, C, K);
    VER_REQUIRE(codes == 8 || codes == 10, VER_EINVAL, "ver_det_decode: codes=%d (8, or 10 with the velocity)", codes);
    VER_REQUIRE(box_ld >= codes, VER_EINVAL, "ver_det_decode: box_ld=%d is below codes=%d", box_ld, codes);
    VER_REQUIRE(cls_dtype == VER_F32 || cls_dtype == VER_BF16, VER_EINVAL, "ver_det_decode: cls_dtype=%d", cls_dtype);
    VER_REQUIRE((flags & ~3) == 0, VER_EINVAL, "ver_det_decode: flags=%d (bit 0: bottom centre, bit 1: score threshold)", flags);
    const long qc = cls ? (long)Q * C : (long)Q;
    if (cls) {
        VER_REQUIRE(K <= qc, VER_EINVAL, "ver_det_decode: K=%d exceeds Q*C=%ld", K, qc);
    } else {
        VER_REQUIRE(K == 0 || K == Q, VER_EINVAL, "ver_det_decode: the layout form (cls == NULL) decodes every query, K=%d Q=%d", K, Q);
    }
    VER_REQUIRE(K <= kDecodeMaxSlots && qc <= kDecodeMaxKeys, VER_EUNSUPPORTED,
                "ver_det_decode: K=%d Q*C=%ld (built for at most %d slots of %d keys)", K, qc, kDecodeMaxSlots, kDecodeMaxKeys);
    if (B == 0 || K == 0) return VER_OK;
    VER_REQUIRE(box && out_boxes && out_scores && out_labels && out_valid && center_range, VER_EINVAL,
                "ver_det_decode: null pointer argument");
    CenterRange rng;
    for (int i = 0; i < 6; ++i) rng.v[i] = center_range[i];
    int n = 1;
    while (n < qc) n <<= 1;
    const int work = cls ? (n / 2 > K ? n / 2 : K) : K;
    int threads = (work + VER_WAVE - 1) / VER_WAVE * VER_WAVE;
    if (threads > kDecodeThreads) threads = kDecodeThreads;
    const size_t lds = cls ? (size_t)n * sizeof(unsigned long long) : 0;
    if (lds > 64 * 1024) {
        if (int rc = ver_lds_limit("ver_det_decode", reinterpret_cast<const void*>(k_det_decode), lds)) return rc;
    }
    hipLaunchKernelGGL(k_det_decode, dim3((unsigned)B), dim3((unsigned)threads), lds, (hipStream_t)stream, cls,
                       cls_dtype == VER_BF16 ? 1 : 0, box, box_ld, out_boxes, out_scores, out_labels, out_valid, out_query, rng,
                       score_threshold, flags, Q, C, K, codes, n);
    return ver_check_launch("ver_det_decode");
}
