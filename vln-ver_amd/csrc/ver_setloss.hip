// Detection set loss on the device (include/ver_ops.h: ver_det_costs, ver_det_set_loss_forward / _backward): the matching
// costs the Hungarian assigner solves, and the focal + L1 terms of every decoder layer with their gradients, straight from
// the decoder's outputs, the padded ground truth and the match ver_lsa_solve wrote.  The torch chain these replace is about
// twenty (costs) plus thirty (targets, losses) small elementwise launches and their autograd replay.
//
// The data is tiny (L * bs * Nq = 115 200 rows of 17 logits and 10 box codes at L = 6, bs = 192), so the work split follows
// the launch count, not bandwidth:
//   k_det_costs     one workgroup per (layer, sample).  The normalised ground truths (transposed, [8][Gcap]) and the labels sit
//                   in LDS; the Q x C table w_cls * (pos - neg) is staged per chunk of queries, so the two logarithms per
//                   (query, class) are taken once, not once per column; then the threads run over (q, g), g fastest.
//   k_set_loss_fwd  one 1024-thread workgroup per layer, in tiles of 1024 rows (a row's thread resolves match -> count ->
//                   label once, the tile's logits are then read classes fastest with the labels out of LDS): the layer's
//                   two sums and its positive count leave the kernel
//                   finished, in ONE fixed order (lane butterfly, then the 16 wave sums in wave order) -- bit-reproducible,
//                   no float atomics, no partials handed between workgroups, no workspace to clear.
//   k_set_loss_bwd  elementwise over tiles of 256 rows, grid-stride: nothing is kept by the forward, the per-row terms are
//                   recomputed, each row's target once.
#include <cmath>
#include "ver_common.h"

namespace {

constexpr int kMaxQ = 1024, kMaxG = 1024, kMaxC = 64;   // Q, Gcap: the solver's own limits
constexpr int kTabFloats = 6144;                        // cost table chunk: 24 KiB beside <= 36 KiB of ground truth
constexpr int kCostThreads = 256, kFwdThreads = 1024, kBwdThreads = 256;

// normalize_bbox (dense_heads/coders.py): (cx, cy, cz, w, l, h, yaw, vx, vy) -> (cx, cy, log w, log l, cz, log h, sin, cos, vx, vy)
template <int N>
__device__ __forceinline__ void normalized_target(const float* __restrict__ g, float (&n)[N]) {
    n[0] = g[0];
    n[1] = g[1];
    n[2] = logf(g[3]);
    n[3] = logf(g[4]);
    n[4] = g[2];
    n[5] = logf(g[5]);
    n[6] = sinf(g[6]);
    n[7] = cosf(g[6]);
    if constexpr (N > 8) {
        n[8] = g[7];
        n[9] = g[8];
    }
}

__device__ __forceinline__ bool finite_f32(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for NaN and +-inf

template <bool BF16>
__device__ __forceinline__ float load_logit(const void* base, size_t i) {
    if (BF16) return bf16_to_f32(static_cast<const uint16_t*>(base)[i]);
    return static_cast<const float*>(base)[i];
}

__device__ __forceinline__ uint16_t to_bf16(float f) {   // round to nearest even
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// FocalLossCost (dense_heads/assigner.py) for one logit: w * (pos - neg), pos = -log(p + eps) alpha (1 - p)^gamma,
// neg = -log(1 - p + eps) (1 - alpha) p^gamma.  p and 1 - p both come from exp(-|x|) without a subtraction, so 1 - p keeps
// its relative precision where p rounds to 1 (the fp32 torch chain loses it there: 5e-5 at a logit of 7).
__device__ __forceinline__ float focal_cost(float x, float w, float alpha, float gamma, float eps) {
    const float e = expf(-fabsf(x));
    const float inv = 1.0f / (1.0f + e), einv = e * inv;
    const float p = x >= 0.0f ? inv : einv, q = x >= 0.0f ? einv : inv;
    const float pg = gamma == 2.0f ? p * p : powf(p, gamma), qg = gamma == 2.0f ? q * q : powf(q, gamma);
    const float neg = -logf(q + eps) * (1.0f - alpha) * pg;
    const float pos = -logf(p + eps) * alpha * qg;
    return (pos - neg) * w;
}

// One element of losses.sigmoid_focal_loss and its derivative: the fp32 (non-FAST) arithmetic of ver_loss.hip's focal_term.
struct Term {
    float loss, grad;
};

template <bool G2>
__device__ __forceinline__ Term focal_term(float x, bool pos, float gamma, float alpha) {
    // log p = -softplus(-x), log(1-p) = -softplus(x); softplus(z) = max(z,0) + log1p(exp(-|z|))
    const float e = __expf(-fabsf(x));
    const float l1p = log1pf(e);
    const float sp_pos = fmaxf(x, 0.0f) + l1p;
    const float sp_neg = fmaxf(-x, 0.0f) + l1p;
    const float inv = 1.0f / (1.0f + e);
    const float p = x >= 0.0f ? inv : e * inv;
    const float q = 1.0f - p;
    Term t;
    if (pos) {
        const float m = G2 ? q * q : powf(q, gamma);
        t.loss = alpha * m * sp_neg;
        t.grad = alpha * m * (-gamma * p * sp_neg - q);
    } else {
        const float m = G2 ? p * p : powf(p, gamma);
        t.loss = (1.0f - alpha) * m * sp_pos;
        t.grad = (1.0f - alpha) * m * (p + gamma * q * sp_pos);
    }
    return t;
}

__device__ __forceinline__ int clamp_count(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

// ------------------------------------------------------------------------------------------------------------ costs
template <bool BF16>
__global__ __launch_bounds__(kCostThreads) void k_det_costs(const void* __restrict__ cls, const float* __restrict__ box, int box_ld,
                                                            const float* __restrict__ gt, const int64_t* __restrict__ gt_labels,
                                                            const int* __restrict__ counts, float* __restrict__ cost, int B, int Q,
                                                            int C, int Gcap, int QT, float w_cls, float alpha, float gamma,
                                                            float eps, float w_reg) {
    extern __shared__ __attribute__((aligned(16))) float costs_smem[];
    float* gtn = costs_smem;                               // [8][Gcap] normalised ground truth, non-finite entries -> 0
    int* lab = reinterpret_cast<int*>(gtn + 8 * Gcap);     // [Gcap]    label, -1 when outside [0, C)
    float* tab = reinterpret_cast<float*>(lab + Gcap);     // [QT][C]   w_cls * (pos - neg) of this chunk of queries

    const int tid = threadIdx.x;
    const size_t p = blockIdx.x;                           // (layer, sample)
    const int b = (int)(p % (size_t)B);
    const int nc = clamp_count(counts[b], Gcap);
    for (int g = tid; g < nc; g += kCostThreads) {
        float n[8];
        normalized_target(gt + ((size_t)b * Gcap + g) * 9, n);
#pragma unroll
        for (int k = 0; k < 8; ++k) gtn[k * Gcap + g] = finite_f32(n[k]) ? n[k] : 0.0f;
        if (cls) {
            const int64_t t = gt_labels[(size_t)b * Gcap + g];
            lab[g] = (t >= 0 && t < C) ? (int)t : -1;
        }
    }
    const float* pbox = box + p * (size_t)Q * box_ld;
    float* pcost = cost + p * (size_t)Q * Gcap;
    for (int q0 = 0; q0 < Q; q0 += QT) {
        const int qt = Q - q0 < QT ? Q - q0 : QT;
        __syncthreads();                                   // the ground truth is staged / the previous chunk's table is read
        if (cls && nc > 0) {
            const size_t base = (p * (size_t)Q + q0) * C;
            for (int i = tid; i < qt * C; i += kCostThreads) tab[i] = focal_cost(load_logit<BF16>(cls, base + i), w_cls, alpha, gamma, eps);
        }
        __syncthreads();
        for (int i = tid; i < qt * Gcap; i += kCostThreads) {
            const int q = i / Gcap, g = i - q * Gcap;
            float out = 0.0f;                              // columns >= counts[b]
            if (g < nc) {
                const float* bq = pbox + (size_t)(q0 + q) * box_ld;
                float reg = 0.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k) reg += fabsf(bq[k] - gtn[k * Gcap + g]);
                reg *= w_reg;
                if (cls) {
                    const int t = lab[g];
                    out = (t >= 0 ? tab[q * C + t] : __builtin_nanf("")) + reg;
                } else {
                    out = reg;
                }
            }
            pcost[(size_t)q0 * Gcap + i] = out;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ loss
// What a row (l, b, q) is matched to.  status: 0 background, 1 matched, -1 a match outside [-1, counts[b]) or a matched label
// outside [0, C) (the layer is poisoned; the row reads nothing through the index).
struct RowTarget {
    int status, label, slot;
    bool nonneg;                                           // match >= 0: what npos counts, valid or not
};

__device__ __forceinline__ RowTarget row_target(const int* __restrict__ match, const int64_t* __restrict__ gt_labels,
                                                const int* __restrict__ counts, size_t row_in_all, int row_in_layer, int Q, int C,
                                                int Gcap, bool with_labels) {
    RowTarget r;
    r.status = 0;
    r.label = C;
    r.slot = 0;
    const int m = match[row_in_all];
    r.nonneg = m >= 0;
    if (m == -1) return r;
    const int b = row_in_layer / Q;
    if (m < -1 || m >= clamp_count(counts[b], Gcap)) {
        r.status = -1;
        return r;
    }
    r.status = 1;
    r.slot = b * Gcap + m;
    if (with_labels) {
        const int64_t t = gt_labels[r.slot];
        if (t < 0 || t >= C) {
            r.status = -1;
            return r;
        }
        r.label = (int)t;
    }
    return r;
}

template <bool BF16, bool G2>
__global__ __launch_bounds__(kFwdThreads) void k_set_loss_fwd(const void* __restrict__ cls, const float* __restrict__ box, int box_ld,
                                                              const int* __restrict__ match, const float* __restrict__ gt,
                                                              const int64_t* __restrict__ gt_labels, const int* __restrict__ counts,
                                                              const float* __restrict__ code_weights, float* __restrict__ sums,
                                                              int* __restrict__ npos, int* __restrict__ bad, int L, int B, int Q,
                                                              int C, int Gcap, float gamma, float alpha) {
    __shared__ float red_f[2][kFwdThreads / VER_WAVE];
    __shared__ int red_i[2][kFwdThreads / VER_WAVE];
    __shared__ int lab_s[kFwdThreads];                     // label of each row of the tile (C: background)
    const int tid = threadIdx.x;
    const int l = blockIdx.x;
    const int rows = B * Q;                                // <= 2^31 / kMaxC, checked by the launcher
    const size_t row0 = (size_t)l * rows;
    float focal = 0.0f, l1 = 0.0f;
    int pos = 0, isbad = 0;

    // tiles of 1024 rows: a row's thread resolves its target ONCE (match -> count -> label) and takes the box term; then
    // the threads run over the tile's logits, classes fastest, with the labels out of LDS
    for (int t0 = 0; t0 < rows; t0 += kFwdThreads) {
        const int r = t0 + tid;
        int label = C;
        if (r < rows) {
            const RowTarget t = row_target(match, gt_labels, counts, row0 + r, r, Q, C, Gcap, cls != nullptr);
            if (t.status < 0) isbad = 1;
            pos += t.nonneg ? 1 : 0;
            if (t.status > 0) {
                label = t.label;
                float n[10];
                normalized_target(gt + (size_t)t.slot * 9, n);
                bool keep = true;
#pragma unroll
                for (int k = 0; k < 10; ++k) keep = keep && finite_f32(n[k]);
                if (keep) {                                // (not kept: the rows the reference drops by boolean indexing)
                    const float* bq = box + (row0 + r) * (size_t)box_ld;
                    float s = 0.0f;
#pragma unroll
                    for (int k = 0; k < 10; ++k) s += code_weights[k] * fabsf(bq[k] - n[k]);
                    l1 += s;
                }
            }
        }
        if (cls) {
            __syncthreads();                               // the previous tile's labels have been read
            lab_s[tid] = label;
            __syncthreads();
            const int elems = (rows - t0 < kFwdThreads ? rows - t0 : kFwdThreads) * C;
            const size_t base = (row0 + t0) * C;
            for (int e = tid; e < elems; e += kFwdThreads) {
                const int rr = e / C, c = e - rr * C;
                focal += focal_term<G2>(load_logit<BF16>(cls, base + e), lab_s[rr] == c, gamma, alpha).loss;
            }
        }
    }
    // fixed order: xor butterfly inside a wave, then the wave sums in wave order
#pragma unroll
    for (int off = VER_WAVE / 2; off > 0; off >>= 1) {
        focal += __shfl_xor(focal, off, VER_WAVE);
        l1 += __shfl_xor(l1, off, VER_WAVE);
        pos += __shfl_xor(pos, off, VER_WAVE);
        isbad |= __shfl_xor(isbad, off, VER_WAVE);
    }
    const int wave = tid / VER_WAVE;
    if ((tid & (VER_WAVE - 1)) == 0) {
        red_f[0][wave] = focal;
        red_f[1][wave] = l1;
        red_i[0][wave] = pos;
        red_i[1][wave] = isbad;
    }
    __syncthreads();
    if (tid == 0) {
        float f = 0.0f, s = 0.0f;
        int n = 0, any = 0;
        for (int w = 0; w < kFwdThreads / VER_WAVE; ++w) {
            f += red_f[0][w];
            s += red_f[1][w];
            n += red_i[0][w];
            any |= red_i[1][w];
        }
        if (any) {
            f = s = __builtin_nanf("");
            if (bad) atomicOr(bad, 1);
        }
        sums[l] = f;
        sums[L + l] = s;
        npos[l] = n;
    }
}

template <bool BF16, bool G2>
__global__ __launch_bounds__(kBwdThreads) void k_set_loss_bwd(const void* __restrict__ cls, const float* __restrict__ box, int box_ld,
                                                              const int* __restrict__ match, const float* __restrict__ gt,
                                                              const int64_t* __restrict__ gt_labels, const int* __restrict__ counts,
                                                              const float* __restrict__ code_weights, const float* __restrict__ scale,
                                                              void* __restrict__ grad_cls, float* __restrict__ grad_box, int L, int B,
                                                              int Q, int C, int Gcap, float gamma, float alpha) {
    __shared__ int lab_s[kBwdThreads];                     // label of each row of the tile (C: background)
    const int tid = threadIdx.x;
    const int rows = B * Q;
    const size_t all_rows = (size_t)L * rows;
    const size_t tiles = (all_rows + kBwdThreads - 1) / kBwdThreads;
    // tiles of 256 rows (a tile may straddle two layers): a row's thread resolves its target once and writes the row's box
    // gradient; then the threads run over the tile's logits, classes fastest, with the labels out of LDS
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t row = tile * kBwdThreads + tid;
        int label = C;
        if (row < all_rows) {
            const int l = (int)(row / rows), r = (int)(row - (size_t)l * rows);
            const float s = scale[L + l];
            const RowTarget t = row_target(match, gt_labels, counts, row, r, Q, C, Gcap, cls != nullptr);
            float* gq = grad_box + row * (size_t)box_ld;
            bool keep = false;
            float n[10];
            if (t.status > 0) {
                label = t.label;
                if (s != 0.0f) {                           // a layer with scale 0: exact zeros, whatever its codes hold
                    normalized_target(gt + (size_t)t.slot * 9, n);
                    keep = true;
#pragma unroll
                    for (int k = 0; k < 10; ++k) keep = keep && finite_f32(n[k]);
                }
            }
            if (keep) {
                const float* bq = box + row * (size_t)box_ld;
#pragma unroll
                for (int k = 0; k < 10; ++k) {
                    const float d = bq[k] - n[k];
                    const float sign = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : d);   // sign(0) = 0 (a NaN code stays NaN)
                    gq[k] = s * code_weights[k] * sign;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 10; ++k) gq[k] = 0.0f;
            }
            for (int k = 10; k < box_ld; ++k) gq[k] = 0.0f;
        }
        if (cls) {
            __syncthreads();                               // the previous tile's labels have been read
            lab_s[tid] = label;
            __syncthreads();
            const size_t first_row = tile * kBwdThreads;
            const int in_tile = all_rows - first_row < (size_t)kBwdThreads ? (int)(all_rows - first_row) : kBwdThreads;
            const size_t base = first_row * C;
            for (int e = tid; e < in_tile * C; e += kBwdThreads) {
                const int rr = e / C, c = e - rr * C;
                const float s = scale[(first_row + rr) / rows];
                float g = 0.0f;                            // a layer with scale 0: exact zeros, whatever its logits hold
                if (s != 0.0f) g = s * focal_term<G2>(load_logit<BF16>(cls, base + e), lab_s[rr] == c, gamma, alpha).grad;
                if (BF16)
                    static_cast<uint16_t*>(grad_cls)[base + e] = to_bf16(g);
                else
                    static_cast<float*>(grad_cls)[base + e] = g;
            }
        }
    }
}

int check_loss_args(const char* what, const void* cls, int cls_dtype, const void* box, int box_ld, const void* match, const void* gt,
                    const void* gt_labels, const void* counts, const void* code_weights, int L, int B, int Q, int C, int Gcap) {
    VER_REQUIRE(L >= 0 && B >= 0 && Q >= 0 && C >= 0 && Gcap >= 0, VER_EINVAL, "%s: bad sizes L=%d B=%d Q=%d C=%d Gcap=%d", what, L, B,
                Q, C, Gcap);
    VER_REQUIRE(box_ld >= 10, VER_EINVAL, "%s: box_ld=%d (the ten box codes are read: box_ld >= 10)", what, box_ld);
    VER_REQUIRE(cls_dtype == VER_F32 || cls_dtype == VER_BF16, VER_EINVAL, "%s: cls_dtype=%d", what, cls_dtype);
    VER_REQUIRE(Q <= kMaxQ && Gcap <= kMaxG && C <= kMaxC, VER_EUNSUPPORTED, "%s: Q=%d Gcap=%d C=%d (built for at most %d, %d, %d)",
                what, Q, Gcap, C, kMaxQ, kMaxG, kMaxC);
    VER_REQUIRE((long)B * Q <= (long)(INT32_MAX / kMaxC), VER_EUNSUPPORTED, "%s: B*Q=%ld rows per layer (at most %d)", what,
                (long)B * Q, INT32_MAX / kMaxC);
    if (L == 0) return VER_OK;
    if ((long)B * Q > 0) {
        VER_REQUIRE(box && match && counts && code_weights, VER_EINVAL, "%s: null pointer argument", what);
        VER_REQUIRE((gt || Gcap == 0) && (!cls || gt_labels || Gcap == 0), VER_EINVAL, "%s: null pointer argument", what);
    }
    return VER_OK;
}

}  // namespace

extern "C" int ver_det_costs(const void* cls, int cls_dtype, const float* box, int box_ld, const float* gt,
                             const int64_t* gt_labels, const int32_t* counts, float* cost, int L, int B, int Q, int C, int Gcap,
                             float w_cls, float alpha, float gamma, float eps, float w_reg, void* stream) {
    VER_REQUIRE(L >= 0 && B >= 0 && Q >= 0 && C >= 0 && Gcap >= 0, VER_EINVAL, "ver_det_costs: bad sizes L=%d B=%d Q=%d C=%d Gcap=%d",
                L, B, Q, C, Gcap);
    VER_REQUIRE(box_ld >= 8, VER_EINVAL, "ver_det_costs: box_ld=%d (eight box codes are read: box_ld >= 8)", box_ld);
    VER_REQUIRE(cls_dtype == VER_F32 || cls_dtype == VER_BF16, VER_EINVAL, "ver_det_costs: cls_dtype=%d", cls_dtype);
    VER_REQUIRE(Q <= kMaxQ && Gcap <= kMaxG && C <= kMaxC, VER_EUNSUPPORTED,
                "ver_det_costs: Q=%d Gcap=%d C=%d (built for at most %d, %d, %d)", Q, Gcap, C, kMaxQ, kMaxG, kMaxC);
    if (L == 0 || B == 0 || Q == 0 || Gcap == 0) return VER_OK;
    VER_REQUIRE(box && gt && counts && cost && (!cls || gt_labels), VER_EINVAL, "ver_det_costs: null pointer argument");
    VER_REQUIRE(!cls || C >= 1, VER_EINVAL, "ver_det_costs: C=%d with class logits", C);
    VER_REQUIRE((long)L * B <= (long)INT32_MAX, VER_EUNSUPPORTED, "ver_det_costs: L*B=%ld problems", (long)L * B);
    const int per_chunk = cls ? kTabFloats / C : Q;
    const int QT = Q < per_chunk ? Q : per_chunk;
    const size_t lds = (size_t)Gcap * 9 * sizeof(float) + (cls ? (size_t)QT * C * sizeof(float) : 0);
    const dim3 grid((unsigned)((long)L * B)), block(kCostThreads);
    if (cls_dtype == VER_BF16)
        hipLaunchKernelGGL(k_det_costs<true>, grid, block, lds, (hipStream_t)stream, cls, box, box_ld, gt, gt_labels, counts, cost, B, Q,
                           C, Gcap, QT, w_cls, alpha, gamma, eps, w_reg);
    else
        hipLaunchKernelGGL(k_det_costs<false>, grid, block, lds, (hipStream_t)stream, cls, box, box_ld, gt, gt_labels, counts, cost, B, Q,
                           C, Gcap, QT, w_cls, alpha, gamma, eps, w_reg);
    return ver_check_launch("ver_det_costs");
}

extern "C" int ver_det_set_loss_forward(const void* cls, int cls_dtype, const float* box, int box_ld, const int32_t* match,
                                        const float* gt, const int64_t* gt_labels, const int32_t* counts,
                                        const float* code_weights, float* sums, int32_t* npos, int32_t* bad, int L, int B, int Q,
                                        int C, int Gcap, float alpha, float gamma, void* stream) {
    const char* what = "ver_det_set_loss_forward";
    const int rc = check_loss_args(what, cls, cls_dtype, box, box_ld, match, gt, gt_labels, counts, code_weights, L, B, Q, C, Gcap);
    if (rc != VER_OK || L == 0) return rc;
    VER_REQUIRE(sums && npos, VER_EINVAL, "%s: null pointer argument", what);
    const dim3 grid((unsigned)L), block(kFwdThreads);
    const bool bf16 = cls_dtype == VER_BF16, g2 = gamma == 2.0f;
#define VER_SETLOSS_FWD(BF, G2)                                                                                                  \
    hipLaunchKernelGGL((k_set_loss_fwd<BF, G2>), grid, block, 0, (hipStream_t)stream, cls, box, box_ld, match, gt, gt_labels, counts, \
                       code_weights, sums, npos, bad, L, B, Q, C, Gcap, gamma, alpha)
    if (bf16 && g2) VER_SETLOSS_FWD(true, true);
    else if (bf16) VER_SETLOSS_FWD(true, false);
    else if (g2) VER_SETLOSS_FWD(false, true);
    else VER_SETLOSS_FWD(false, false);
#undef VER_SETLOSS_FWD
    return ver_check_launch(what);
}

extern "C" int ver_det_set_loss_backward(const void* cls, int cls_dtype, const float* box, int box_ld, const int32_t* match,
                                         const float* gt, const int64_t* gt_labels, const int32_t* counts,
                                         const float* code_weights, const float* scale, void* grad_cls, float* grad_box, int L,
                                         int B, int Q, int C, int Gcap, float alpha, float gamma, void* stream) {
    const char* what = "ver_det_set_loss_backward";
    const int rc = check_loss_args(what, cls, cls_dtype, box, box_ld, match, gt, gt_labels, counts, code_weights, L, B, Q, C, Gcap);
    if (rc != VER_OK) return rc;
    const size_t all_rows = (size_t)L * B * Q;
    if (all_rows == 0) return VER_OK;
    VER_REQUIRE(scale && grad_box && (!cls || grad_cls), VER_EINVAL, "%s: null pointer argument", what);
    size_t blocks = (all_rows + kBwdThreads - 1) / kBwdThreads;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks), block(kBwdThreads);
    const bool bf16 = cls_dtype == VER_BF16, g2 = gamma == 2.0f;
#define VER_SETLOSS_BWD(BF, G2)                                                                                                  \
    hipLaunchKernelGGL((k_set_loss_bwd<BF, G2>), grid, block, 0, (hipStream_t)stream, cls, box, box_ld, match, gt, gt_labels, counts, \
                       code_weights, scale, grad_cls, grad_box, L, B, Q, C, Gcap, gamma, alpha)
    if (bf16 && g2) VER_SETLOSS_BWD(true, true);
    else if (bf16) VER_SETLOSS_BWD(true, false);
    else if (g2) VER_SETLOSS_BWD(false, true);
    else VER_SETLOSS_BWD(false, false);
#undef VER_SETLOSS_BWD
    return ver_check_launch(what);
}
