// Softmax self-attention of the detection decoder between the input projections and out_proj, forward and backward, one
// launch each way (include/ver_ops.h, ver_mha_*).
//
// nn.MultiheadAttention with need_weights=True runs, per decoder layer and under training, head transposes with copies, the
// q scaling, bmm, softmax, dropout, bmm, a transpose back and a head average nobody reads -- and autograd replays all of it.
// The work of one (sample, head) is 100 x 100 x 96: it fits a workgroup's LDS.  Here one workgroup owns one (sample, head)
// each way, reads q / k / v in the [N, B, heads*head_dim] layout (with a row pitch) the Linears leave them in, and writes
// out / the three gradients in that layout too.  No atomics, no workspace: every output element is written once, by one
// wave, in a fixed summation order.
//
// bf16 operands (k_mha_fwd_bf16 / k_mha_bwd_bf16, 8 waves): the products run on v_mfma_f32_16x16x32_bf16.  Wave w owns the
// 16-row tile w of whatever a product's rows are (queries for S, dPd, out, dQ; keys for dV, dK), so Nq, Nk <= 128 need no
// loop over row tiles.  q, k, v (and dO) are staged row-major [n][d] in LDS, zero padded to 32 rows / 32 columns.  A
// fragment whose 8 k-elements are contiguous in such an image is one 16-byte read (frag_rows); the B operand of a product
// that sums over an image's ROW index (V in P V, dO in Pd^T dO, K in dS K, Q in dS^T Q) is gathered by eight 2-byte reads
// (frag_cols) -- the work is tiny, and it saves a transposed copy of every operand, which is what keeps the backward inside
// 160 KiB at the upper corner.  An accumulator tile holds 4 consecutive rows of one column per lane, so the TRANSPOSED
// images Pd^T [j][i] and dS^T [j][i] are written with one 8-byte store per tile and lane.
// Backward phases (buffers b0 = Q, b1 = K, b2 = V, b3 = dO):
//   1  S = Q K^T and dPd = dO V^T for the wave's query tile -> P, Pd, dP, delta = sum_j dP P, dS, all in registers
//   2  Pd^T -> b2 (V is dead);  dV = Pd^T dO
//   3  dS -> b3 (dO is dead), dS^T -> b2;  dQ = dS K / sqrt(hd),  dK = dS^T Q / sqrt(hd)
//
// fp32 operands (k_mha_fwd_f32 / k_mha_bwd_f32, 4 waves): the parity configuration.  fp32 VALU products with the operands
// read from global memory (L1 / L2 resident), the [Nq, Nk] matrices (P; P and dS backward) in LDS.
#include "ver_common.h"

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxN = 128;        // queries, keys
constexpr int kMaxHd = 128;
constexpr int kTiles = 8;         // 16-wide tiles of the largest dimension = waves of the bf16 kernels
constexpr int kMfmaThreads = 64 * kTiles;
constexpr int kF32Threads = 256;

__host__ __device__ inline int pad32(int n) { return (n + 31) & ~31; }

// LDS bytes of the four kernels (host and device agree through these)
__host__ __device__ inline int mha_ld(int n) { return pad32(n) + 8; }          // bf16 image row pitch, in elements
__host__ __device__ inline size_t lds_fwd_bf16(int hd, int Nq, int Nk) {
    return 2 * ((size_t)pad32(Nq) * mha_ld(hd) + 2 * (size_t)pad32(Nk) * mha_ld(hd) + (size_t)pad32(Nq) * mha_ld(Nk));
}
__host__ __device__ inline int max_i(int a, int b) { return a > b ? a : b; }
__host__ __device__ inline size_t lds_bwd_bf16(int hd, int Nq, int Nk) {
    return 2 * ((size_t)pad32(Nq) * mha_ld(hd) + (size_t)pad32(Nk) * mha_ld(hd) +
                (size_t)pad32(Nk) * max_i(mha_ld(hd), mha_ld(Nq)) + (size_t)pad32(Nq) * max_i(mha_ld(hd), mha_ld(Nk)));
}
__host__ __device__ inline size_t lds_fwd_f32(int Nq, int Nk) { return sizeof(float) * (size_t)Nq * (Nk + 1); }
__host__ __device__ inline size_t lds_bwd_f32(int Nq, int Nk) { return 2 * lds_fwd_f32(Nq, Nk); }

__device__ __forceinline__ uint32_t mha_bf(float f) {   // round to nearest even
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

struct Drop {
    bool on;
    uint64_t seed;
    uint32_t thresh;
    float inv;           // 1 / (1 - p)
    __device__ Drop(const int64_t* seed_p, float p) {
        on = p > 0.0f;
        seed = on ? (uint64_t)seed_p[0] : 0ull;
        thresh = (uint32_t)((1.0f - p) * 16777216.0f);
        inv = on ? 1.0f / (1.0f - p) : 1.0f;
    }
    __device__ __forceinline__ bool keep(uint64_t idx) const { return !on || keep_elem(idx, seed, thresh); }
};

// ------------------------------------------------------------------------------------------ bf16: staging and fragments
// Rows [n][hd] of one (sample, head) -- `src` points at its first element, consecutive rows are `row_stride` elements
// apart -- into the LDS image dst[np][ld], zero padded to np rows and hdp columns.  16-byte pieces: hd % 8 == 0.
__device__ __forceinline__ void stage_rows(uint16_t* dst, int ld, const uint16_t* __restrict__ src, long row_stride, int n,
                                           int np, int hd, int hdp) {
    const int chunks = hdp >> 3;
    for (int e = threadIdx.x; e < np * chunks; e += kMfmaThreads) {
        const int r = e / chunks, c = (e - r * chunks) << 3;
        uint4 t = make_uint4(0u, 0u, 0u, 0u);
        if (r < n && c < hd) t = *reinterpret_cast<const uint4*>(src + (long)r * row_stride + c);
        *reinterpret_cast<uint4*>(dst + r * ld + c) = t;
    }
}

// Fragment element j = m[row0 + (lane & 15)][k0 + 8 (lane >> 4) + j]: the A operand of a row-major image, or the B operand
// of an image held as [column][k].
__device__ __forceinline__ bf16x8 frag_rows(const uint16_t* m, int ld, int row0, int k0, int lane) {
    const uint4 t = *reinterpret_cast<const uint4*>(m + (row0 + (lane & 15)) * ld + k0 + 8 * (lane >> 4));
    return __builtin_bit_cast(bf16x8, t);
}

// Fragment element j = m[k0 + 8 (lane >> 4) + j][col0 + (lane & 15)]: the B operand of a row-major image [k][column].
__device__ __forceinline__ bf16x8 frag_cols(const uint16_t* m, int ld, int k0, int col0, int lane) {
    const uint16_t* p = m + (k0 + 8 * (lane >> 4)) * ld + col0 + (lane & 15);
    uint4 t;
    t.x = (uint32_t)p[0] | ((uint32_t)p[ld] << 16);
    t.y = (uint32_t)p[2 * ld] | ((uint32_t)p[3 * ld] << 16);
    t.z = (uint32_t)p[4 * ld] | ((uint32_t)p[5 * ld] << 16);
    t.w = (uint32_t)p[6 * ld] | ((uint32_t)p[7 * ld] << 16);
    return __builtin_bit_cast(bf16x8, t);
}

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// acc[t] += A[row0 .. row0+15][0 .. depth) * B, t < ntiles, where B is a row-major image [k][column] (frag_cols)
__device__ __forceinline__ void product_cols(f32x4 (&acc)[kTiles], const uint16_t* a, int lda, int row0, const uint16_t* b,
                                             int ldb, int depth, int ntiles, int lane) {
    for (int k0 = 0; k0 < depth; k0 += 32) {
        const bf16x8 af = frag_rows(a, lda, row0, k0, lane);
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
            if (t < ntiles) acc[t] = mfma(af, frag_cols(b, ldb, k0, 16 * t, lane), acc[t]);
    }
}

// An accumulator tile's 4 consecutive rows of column (lane & 15) as 4 packed bf16: one 8-byte store into a [column][row] image
__device__ __forceinline__ void store_transposed(uint16_t* img, int ld, int col, int row, const f32x4& v) {
    uint2 t;
    t.x = mha_bf(v[0]) | (mha_bf(v[1]) << 16);
    t.y = mha_bf(v[2]) | (mha_bf(v[3]) << 16);
    *reinterpret_cast<uint2*>(img + col * ld + row) = t;
}

// dst[(row, b), h*hd + d] = acc * mul of the tile rows row0 .. row0+15 below `n`: lane (lane & 15) has column d, 4 rows
__device__ __forceinline__ void store_rows(uint16_t* __restrict__ dst, long row_stride, const f32x4 (&acc)[kTiles], int row0,
                                           int n, int hd, float mul, int lane) {
    const int c = lane & 15, rq = (lane >> 4) * 4;
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
        const int d = 16 * t + c;
        if (d < hd) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + rq + r < n) dst[(long)(row0 + rq + r) * row_stride + d] = (uint16_t)mha_bf(acc[t][r] * mul);
        }
    }
}
}  // namespace

// ------------------------------------------------------------------------------------------ bf16 forward
__global__ __launch_bounds__(kMfmaThreads) void k_mha_fwd_bf16(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
                                                               const uint16_t* __restrict__ v, long ldq, long ldk, long ldv,
                                                               const int64_t* __restrict__ seed_p, float p_drop,
                                                               uint16_t* __restrict__ out, float* __restrict__ lse, int B,
                                                               int heads, int hd, int Nq, int Nk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mha_smem[];
    const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nqp = pad32(Nq), nkp = pad32(Nk), hdp = pad32(hd);
    const int ldh = mha_ld(hd), ldp = mha_ld(Nk);
    uint16_t* sq = reinterpret_cast<uint16_t*>(mha_smem);
    uint16_t* sk = sq + nqp * ldh;
    uint16_t* sv = sk + nkp * ldh;
    uint16_t* sp = sv + nkp * ldh;                 // P (dropped out), [nqp][ldp]; rows of tile w belong to wave w
    const long C = (long)heads * hd;
    stage_rows(sq, ldh, q + b * ldq + h * hd, B * ldq, Nq, nqp, hd, hdp);
    stage_rows(sk, ldh, k + b * ldk + h * hd, B * ldk, Nk, nkp, hd, hdp);
    stage_rows(sv, ldh, v + b * ldv + h * hd, B * ldv, Nk, nkp, hd, hdp);
    __syncthreads();
    const Drop drop(seed_p, p_drop);
    const float scale = 1.0f / sqrtf((float)hd);
    const int row0 = 16 * w, nkt = nkp >> 4, ndt = (hd + 15) >> 4;
    const int c = lane & 15, rq = (lane >> 4) * 4;
    const bool active = row0 < Nq;
    if (active) {
        f32x4 s[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) s[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int k0 = 0; k0 < hdp; k0 += 32) {
            const bf16x8 af = frag_rows(sq, ldh, row0, k0, lane);
#pragma unroll
            for (int t = 0; t < kTiles; ++t)
                if (t < nkt) s[t] = mfma(af, frag_rows(sk, ldh, 16 * t, k0, lane), s[t]);
        }
        // softmax over the keys: row (rq + r) of the tile lives in register r of the 16 lanes with this lane >> 4
        float mx[4], sum[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = -INFINITY, sum[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
            if (t < nkt) {
                const bool real = 16 * t + c < Nk;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[t][r] = real ? s[t][r] * scale : -INFINITY;
                    mx[r] = fmaxf(mx[r], s[t][r]);
                }
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = group_max<16>(mx[r]);
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
            if (t < nkt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[t][r] = expf(s[t][r] - mx[r]);
                    sum[r] += s[t][r];
                }
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sum[r] = group_sum<16>(sum[r]);
            const int i = row0 + rq + r;
            if (c == 0 && i < Nq) lse[(long)bh * Nq + i] = mx[r] + logf(sum[r]);
            sum[r] = 1.0f / sum[r];
        }
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
            if (t < nkt) {
                const int j = 16 * t + c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = row0 + rq + r;
                    float p = s[t][r] * sum[r];
                    if (drop.on) p = drop.keep(((uint64_t)bh * Nq + i) * Nk + j) ? p * drop.inv : 0.0f;
                    sp[i * ldp + j] = (uint16_t)mha_bf(p);
                }
            }
    }
    __syncthreads();
    if (active) {
        f32x4 o[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) o[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        product_cols(o, sp, ldp, row0, sv, ldh, nkp, ndt, lane);
        store_rows(out + b * C + h * hd, B * C, o, row0, Nq, hd, 1.0f, lane);
    }
}

// ------------------------------------------------------------------------------------------ bf16 backward
__global__ __launch_bounds__(kMfmaThreads) void k_mha_bwd_bf16(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, long ldq, long ldk, long ldv,
    const uint16_t* __restrict__ go, const float* __restrict__ lse, const int64_t* __restrict__ seed_p, float p_drop,
    uint16_t* __restrict__ gq, uint16_t* __restrict__ gk, uint16_t* __restrict__ gv, long ldgq, long ldgk, long ldgv, int B,
    int heads, int hd, int Nq, int Nk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mha_smem[];
    const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nqp = pad32(Nq), nkp = pad32(Nk), hdp = pad32(hd);
    const int ldh = mha_ld(hd), ldi = mha_ld(Nq), ldj = mha_ld(Nk);      // pitches of [.][d], [j][i] and [i][j] images
    uint16_t* b0 = reinterpret_cast<uint16_t*>(mha_smem);                // Q [nqp][ldh]
    uint16_t* b1 = b0 + nqp * ldh;                                        // K [nkp][ldh]
    uint16_t* b2 = b1 + nkp * ldh;                                        // V [nkp][ldh], then Pd^T, then dS^T [nkp][ldi]
    uint16_t* b3 = b2 + nkp * max_i(ldh, ldi);                            // dO [nqp][ldh], then dS [nqp][ldj]
    const long C = (long)heads * hd;
    stage_rows(b0, ldh, q + b * ldq + h * hd, B * ldq, Nq, nqp, hd, hdp);
    stage_rows(b1, ldh, k + b * ldk + h * hd, B * ldk, Nk, nkp, hd, hdp);
    stage_rows(b2, ldh, v + b * ldv + h * hd, B * ldv, Nk, nkp, hd, hdp);
    stage_rows(b3, ldh, go + b * C + h * hd, B * C, Nq, nqp, hd, hdp);
    __syncthreads();
    const Drop drop(seed_p, p_drop);
    const float scale = 1.0f / sqrtf((float)hd);
    const int row0 = 16 * w, nkt = nkp >> 4, ndt = (hd + 15) >> 4;
    const int c = lane & 15, rq = (lane >> 4) * 4;
    const bool q_tile = row0 < nqp;           // padded query rows are computed too: they put zeros into the [j][i] images
    // phase 1: Pd (-> pd) and dS (-> ds) of the wave's 16 queries against every key, in registers
    f32x4 pd[kTiles], ds[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) pd[t] = ds[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (q_tile) {
        f32x4 p[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) p[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int k0 = 0; k0 < hdp; k0 += 32) {
            const bf16x8 aq = frag_rows(b0, ldh, row0, k0, lane), ag = frag_rows(b3, ldh, row0, k0, lane);
#pragma unroll
            for (int t = 0; t < kTiles; ++t)
                if (t < nkt) {
                    p[t] = mfma(aq, frag_rows(b1, ldh, 16 * t, k0, lane), p[t]);        // S
                    ds[t] = mfma(ag, frag_rows(b2, ldh, 16 * t, k0, lane), ds[t]);      // dPd
                }
        }
        float l[4], delta[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = row0 + rq + r;
            l[r] = i < Nq ? lse[(long)bh * Nq + i] : 0.0f;
            delta[r] = 0.0f;
        }
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
            if (t < nkt) {
                const int j = 16 * t + c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = row0 + rq + r;
                    const bool real = i < Nq && j < Nk;
                    const float pr = real ? expf(p[t][r] * scale - l[r]) : 0.0f;
                    const bool keep = drop.keep(((uint64_t)bh * Nq + i) * Nk + j);
                    const float dp = keep ? ds[t][r] * drop.inv : 0.0f;
                    p[t][r] = pr;
                    pd[t][r] = keep ? pr * drop.inv : 0.0f;
                    ds[t][r] = dp;
                    delta[r] += dp * pr;
                }
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) delta[r] = group_sum<16>(delta[r]);
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) ds[t][r] = p[t][r] * (ds[t][r] - delta[r]);
    }
    __syncthreads();                          // every wave is done with V
    // phase 2: dV = Pd^T dO
    if (q_tile) {
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
            if (t < nkt) store_transposed(b2, ldi, 16 * t + c, row0 + rq, pd[t]);
    }
    __syncthreads();
    if (row0 < Nk) {
        f32x4 acc[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        product_cols(acc, b2, ldi, row0, b3, ldh, nqp, ndt, lane);
        store_rows(gv + b * ldgv + h * hd, B * ldgv, acc, row0, Nk, hd, 1.0f, lane);
    }
    __syncthreads();                          // every wave is done with dO and Pd^T
    // phase 3: dQ = dS K / sqrt(hd), dK = dS^T Q / sqrt(hd)
    if (q_tile) {
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
            if (t < nkt) {
                store_transposed(b2, ldi, 16 * t + c, row0 + rq, ds[t]);
#pragma unroll
                for (int r = 0; r < 4; ++r) b3[(row0 + rq + r) * ldj + 16 * t + c] = (uint16_t)mha_bf(ds[t][r]);
            }
    }
    __syncthreads();
    if (row0 < Nq) {
        f32x4 acc[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        product_cols(acc, b3, ldj, row0, b1, ldh, nkp, ndt, lane);
        store_rows(gq + b * ldgq + h * hd, B * ldgq, acc, row0, Nq, hd, scale, lane);
    }
    if (row0 < Nk) {
        f32x4 acc[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        product_cols(acc, b2, ldi, row0, b0, ldh, nqp, ndt, lane);
        store_rows(gk + b * ldgk + h * hd, B * ldgk, acc, row0, Nk, hd, scale, lane);
    }
}

// ------------------------------------------------------------------------------------------ fp32
namespace {
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, VER_WAVE));
    return v;
}

// sum_d a[d] * b[d], d < hd (a multiple of 8; both rows 16-byte aligned): four chains, joined in a fixed order
__device__ __forceinline__ float dot_rows(const float* __restrict__ a, const float* __restrict__ b, int hd) {
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (int d = 0; d < hd; d += 4) {
        const float4 x = *reinterpret_cast<const float4*>(a + d), y = *reinterpret_cast<const float4*>(b + d);
        s0 = fmaf(x.x, y.x, s0);
        s1 = fmaf(x.y, y.y, s1);
        s2 = fmaf(x.z, y.z, s2);
        s3 = fmaf(x.w, y.w, s3);
    }
    return (s0 + s1) + (s2 + s3);
}

// dst[(r, b), d] = mul * sum_n m(n, r) * src[(n, b), d] for r < rows, d < hd; m(n, r) = mat[n * sn + r * sr] in LDS.
// Consecutive threads take consecutive d: the global reads are coalesced, the LDS reads broadcasts.
__device__ __forceinline__ void mat_times_rows(float* __restrict__ dst, long dst_stride, const float* mat, int sn, int sr,
                                               const float* __restrict__ src, long src_stride, int rows, int depth, int hd,
                                               float mul) {
    for (int e = threadIdx.x; e < rows * hd; e += kF32Threads) {
        const int r = e / hd, d = e - r * hd;
        float acc = 0.0f;
        for (int n = 0; n < depth; ++n) acc = fmaf(mat[n * sn + r * sr], src[(long)n * src_stride + d], acc);
        dst[(long)r * dst_stride + d] = acc * mul;
    }
}
}  // namespace

__global__ __launch_bounds__(kF32Threads) void k_mha_fwd_f32(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, long ldq, long ldk, long ldv,
                                                             const int64_t* __restrict__ seed_p, float p_drop,
                                                             float* __restrict__ out, float* __restrict__ lse, int B, int heads,
                                                             int hd, int Nq, int Nk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mha_smem[];
    float* P = reinterpret_cast<float*>(mha_smem);                        // [Nq][Nk + 1]
    const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ld = Nk + 1;
    const long C = (long)heads * hd;
    const float* qb = q + b * ldq + h * hd;
    const float* kb = k + b * ldk + h * hd;
    const Drop drop(seed_p, p_drop);
    const float scale = 1.0f / sqrtf((float)hd);
    for (int e = threadIdx.x; e < Nq * Nk; e += kF32Threads) {
        const int i = e / Nk, j = e - i * Nk;
        P[i * ld + j] = dot_rows(qb + (long)i * B * ldq, kb + (long)j * B * ldk, hd) * scale;
    }
    __syncthreads();
    for (int i = w; i < Nq; i += kF32Threads / VER_WAVE) {                // one wave per row
        float mx = -INFINITY, sum = 0.0f;
        for (int j = lane; j < Nk; j += VER_WAVE) mx = fmaxf(mx, P[i * ld + j]);
        mx = wave_max(mx);
        for (int j = lane; j < Nk; j += VER_WAVE) sum += expf(P[i * ld + j] - mx);
        sum = group_sum<64>(sum);
        if (lane == 0) lse[(long)bh * Nq + i] = mx + logf(sum);
        const float inv = 1.0f / sum;
        for (int j = lane; j < Nk; j += VER_WAVE) {
            const float p = expf(P[i * ld + j] - mx) * inv;
            P[i * ld + j] = drop.keep(((uint64_t)bh * Nq + i) * Nk + j) ? p * drop.inv : 0.0f;
        }
    }
    __syncthreads();
    mat_times_rows(out + b * C + h * hd, B * C, P, 1, ld, v + b * ldv + h * hd, B * ldv, Nq, Nk, hd, 1.0f);
}

__global__ __launch_bounds__(kF32Threads) void k_mha_bwd_f32(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long ldq, long ldk, long ldv,
    const float* __restrict__ go, const float* __restrict__ lse, const int64_t* __restrict__ seed_p, float p_drop,
    float* __restrict__ gq, float* __restrict__ gk, float* __restrict__ gv, long ldgq, long ldgk, long ldgv, int B, int heads,
    int hd, int Nq, int Nk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mha_smem[];
    const int ld = Nk + 1;
    float* P = reinterpret_cast<float*>(mha_smem);                        // [Nq][ld]: P, then Pd
    float* D = P + Nq * ld;                                               // [Nq][ld]: dP, then dS
    const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long C = (long)heads * hd;
    const float* qb = q + b * ldq + h * hd;
    const float* kb = k + b * ldk + h * hd;
    const float* vb = v + b * ldv + h * hd;
    const float* gob = go + b * C + h * hd;
    const Drop drop(seed_p, p_drop);
    const float scale = 1.0f / sqrtf((float)hd);
    for (int e = threadIdx.x; e < Nq * Nk; e += kF32Threads) {
        const int i = e / Nk, j = e - i * Nk;
        const float s = dot_rows(qb + (long)i * B * ldq, kb + (long)j * B * ldk, hd) * scale;
        const float g = dot_rows(gob + (long)i * B * C, vb + (long)j * B * ldv, hd);
        P[i * ld + j] = expf(s - lse[(long)bh * Nq + i]);
        D[i * ld + j] = drop.keep(((uint64_t)bh * Nq + i) * Nk + j) ? g * drop.inv : 0.0f;
    }
    __syncthreads();
    for (int i = w; i < Nq; i += kF32Threads / VER_WAVE) {
        float delta = 0.0f;
        for (int j = lane; j < Nk; j += VER_WAVE) delta = fmaf(D[i * ld + j], P[i * ld + j], delta);
        delta = group_sum<64>(delta);
        for (int j = lane; j < Nk; j += VER_WAVE) {
            const float p = P[i * ld + j];
            D[i * ld + j] = p * (D[i * ld + j] - delta);
            P[i * ld + j] = drop.keep(((uint64_t)bh * Nq + i) * Nk + j) ? p * drop.inv : 0.0f;
        }
    }
    __syncthreads();
    mat_times_rows(gv + b * ldgv + h * hd, B * ldgv, P, ld, 1, gob, B * C, Nk, Nq, hd, 1.0f);          // dV = Pd^T dO
    mat_times_rows(gk + b * ldgk + h * hd, B * ldgk, D, ld, 1, qb, B * ldq, Nk, Nq, hd, scale);        // dK = dS^T Q
    mat_times_rows(gq + b * ldgq + h * hd, B * ldgq, D, 1, ld, kb, B * ldk, Nq, Nk, hd, scale);        // dQ = dS K
}

// ------------------------------------------------------------------------------------------ host
namespace {
bool shape_supported(int B, int heads, int hd, int Nq, int Nk) {
    return B >= 0 && heads >= 1 && Nq >= 1 && Nq <= kMaxN && Nk >= 1 && Nk <= kMaxN && hd >= 8 && hd <= kMaxHd && hd % 8 == 0 &&
           (long)B * heads < (1L << 31);
}

bool pitch_ok(long ld, long C) { return ld % 8 == 0 && ld >= C; }

// VER_OK with *launch = false: nothing to do.  The order is the contract: dtype and signs, the empty call, null pointers,
// the supported range, alignment.
int check_mha(const char* who, bool all_pointers, const int64_t* seed, int dtype, float p_drop, const long* pitch, int npitch,
              const void* const* aligned, int naligned, int B, int heads, int hd, int Nq, int Nk, bool* launch) {
    *launch = false;
    VER_REQUIRE(dtype == VER_F32 || dtype == VER_BF16, VER_EINVAL, "%s: dtype %d is neither VER_F32 nor VER_BF16", who, dtype);
    VER_REQUIRE(B >= 0 && heads >= 1 && hd >= 1 && Nq >= 0 && Nk >= 0, VER_EINVAL,
                "%s: B %d, heads %d, head_dim %d, Nq %d, Nk %d: a negative or zero size", who, B, heads, hd, Nq, Nk);
    if (B == 0 || Nq == 0) return VER_OK;
    VER_REQUIRE(Nk > 0, VER_EINVAL, "%s: %d queries and no key", who, Nq);
    VER_REQUIRE(all_pointers, VER_EINVAL, "%s: null pointer argument", who);
    VER_REQUIRE(p_drop >= 0.0f && p_drop < 1.0f, VER_EUNSUPPORTED, "%s: dropout probability %g outside [0, 1)", who, p_drop);
    VER_REQUIRE(seed || p_drop == 0.0f, VER_EINVAL, "%s: null seed pointer with p_drop %g", who, p_drop);
    VER_REQUIRE(Nq <= kMaxN && Nk <= kMaxN, VER_EUNSUPPORTED, "%s: Nq %d, Nk %d: at most %d queries and %d keys", who, Nq, Nk,
                kMaxN, kMaxN);
    VER_REQUIRE(hd % 8 == 0 && hd <= kMaxHd, VER_EUNSUPPORTED, "%s: head_dim %d: a multiple of 8 up to %d", who, hd, kMaxHd);
    VER_REQUIRE((long)B * heads < (1L << 31), VER_EUNSUPPORTED, "%s: B * heads = %ld: below 2^31", who, (long)B * heads);
    for (int i = 0; i < npitch; ++i)
        VER_REQUIRE(pitch_ok(pitch[i], (long)heads * hd), VER_EUNSUPPORTED,
                    "%s: row pitch %ld: a multiple of 8 and at least heads * head_dim = %ld", who, pitch[i], (long)heads * hd);
    for (int i = 0; i < naligned; ++i)
        VER_REQUIRE(((uintptr_t)aligned[i] & 15) == 0, VER_EINVAL, "%s: operands must be 16-byte aligned", who);
    *launch = true;
    return VER_OK;
}

int grow_lds(const char* who, const void* kern, size_t lds) {
    return lds <= 64 * 1024 ? VER_OK : ver_lds_limit(who, kern, lds);
}
}  // namespace

extern "C" int ver_mha_supported(int B, int heads, int head_dim, int Nq, int Nk) {
    static_assert(2 * (4 * (size_t)kMaxN * (kMaxN + 8)) <= 160 * 1024, "bf16 images of the upper corner exceed the LDS");
    static_assert(2 * sizeof(float) * kMaxN * (kMaxN + 1) <= 160 * 1024, "fp32 matrices of the upper corner exceed the LDS");
    return shape_supported(B, heads, head_dim, Nq, Nk) ? 1 : 0;
}

extern "C" int ver_mha_forward(const void* q, const void* k, const void* v, int dtype, long ldq, long ldk, long ldv,
                               const int64_t* seed, float p_drop, void* out, float* lse, int B, int heads, int head_dim, int Nq,
                               int Nk, void* stream) {
    const char* who = "ver_mha_forward";
    const long pitch[3] = {ldq, ldk, ldv};
    const void* const aligned[3] = {q, k, v};
    bool launch;
    const int rc = check_mha(who, q && k && v && out && lse, seed, dtype, p_drop, pitch, 3, aligned, 3, B, heads, head_dim, Nq,
                             Nk, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long)B * heads));
    if (dtype == VER_BF16) {
        const size_t lds = lds_fwd_bf16(head_dim, Nq, Nk);
        if (int e = grow_lds(who, reinterpret_cast<const void*>(k_mha_fwd_bf16), lds)) return e;
        hipLaunchKernelGGL(k_mha_fwd_bf16, grid, dim3(kMfmaThreads), lds, st, (const uint16_t*)q, (const uint16_t*)k,
                           (const uint16_t*)v, ldq, ldk, ldv, seed, p_drop, (uint16_t*)out, lse, B, heads, head_dim, Nq, Nk);
    } else {
        const size_t lds = lds_fwd_f32(Nq, Nk);
        if (int e = grow_lds(who, reinterpret_cast<const void*>(k_mha_fwd_f32), lds)) return e;
        hipLaunchKernelGGL(k_mha_fwd_f32, grid, dim3(kF32Threads), lds, st, (const float*)q, (const float*)k, (const float*)v,
                           ldq, ldk, ldv, seed, p_drop, (float*)out, lse, B, heads, head_dim, Nq, Nk);
    }
    return ver_check_launch(who);
}

extern "C" int ver_mha_backward(const void* q, const void* k, const void* v, int dtype, long ldq, long ldk, long ldv,
                                const void* grad_out, const float* lse, const int64_t* seed, float p_drop, void* grad_q,
                                void* grad_k, void* grad_v, long ldgq, long ldgk, long ldgv, int B, int heads, int head_dim,
                                int Nq, int Nk, void* stream) {
    const char* who = "ver_mha_backward";
    const long pitch[6] = {ldq, ldk, ldv, ldgq, ldgk, ldgv};
    const void* const aligned[4] = {q, k, v, grad_out};
    bool launch;
    const int rc = check_mha(who, q && k && v && grad_out && lse && grad_q && grad_k && grad_v, seed, dtype, p_drop, pitch, 6,
                             aligned, 4, B, heads, head_dim, Nq, Nk, &launch);
    if (rc || !launch) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long)B * heads));
    if (dtype == VER_BF16) {
        const size_t lds = lds_bwd_bf16(head_dim, Nq, Nk);
        if (int e = grow_lds(who, reinterpret_cast<const void*>(k_mha_bwd_bf16), lds)) return e;
        hipLaunchKernelGGL(k_mha_bwd_bf16, grid, dim3(kMfmaThreads), lds, st, (const uint16_t*)q, (const uint16_t*)k,
                           (const uint16_t*)v, ldq, ldk, ldv, (const uint16_t*)grad_out, lse, seed, p_drop, (uint16_t*)grad_q,
                           (uint16_t*)grad_k, (uint16_t*)grad_v, ldgq, ldgk, ldgv, B, heads, head_dim, Nq, Nk);
    } else {
        const size_t lds = lds_bwd_f32(Nq, Nk);
        if (int e = grow_lds(who, reinterpret_cast<const void*>(k_mha_bwd_f32), lds)) return e;
        hipLaunchKernelGGL(k_mha_bwd_f32, grid, dim3(kF32Threads), lds, st, (const float*)q, (const float*)k, (const float*)v,
                           ldq, ldk, ldv, (const float*)grad_out, lse, seed, p_drop, (float*)grad_q, (float*)grad_k,
                           (float*)grad_v, ldgq, ldgk, ldgv, B, heads, head_dim, Nq, Nk);
    }
    return ver_check_launch(who);
}
