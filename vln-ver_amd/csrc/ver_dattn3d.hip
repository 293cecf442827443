// Detection decoder's 3-D deformable attention between its input Linears and output_proj, one launch forward and two
// backward: ver_dattn3d_forward / ver_dattn3d_backward (include/ver_ops.h).
//
// The reference's VoxelCustomMSDeformableAttention.forward (bevformer/modules/voxel_decoder.py:234-337) takes a softmax over
// the (level, point) logits of a (query, head), builds loc = reference_point + offset / (W, H, D) and samples the value volume
// trilinearly (voxel_temporal_self_attention.py:275-335).  ver_msda3d_* start after the softmax and the location arithmetic;
// these kernels start at the raw Linear outputs, as ver_sca_* do for the encoder.
//
//   k_dattn3d_fwd    one aligned group of G lanes per (b, q, head), lanes over the head_dim channels (the organisation of
//                    k_msda3d_fwd); every lane of the group walks the <= 32 logits for the softmax statistics itself.
//   k_dattn3d_bwd_q  one workgroup per (b, q), its groups over the heads: d(attention weight) and d(loc) of every sample as
//                    k_msda3d_bwd forms them, left in LDS; after one barrier the softmax backward, the division by
//                    (W, H, D) and the head / point sum of grad_ref run on them in a fixed order.
//   k_dattn3d_bwd_v  grad_value as a GATHER: a workgroup owns 64 keys of one (b, head), each of its four waves 16 of them
//                    with an fp32 accumulator tile in LDS.  The workgroup lists the (key, softmax weight * corner weight)
//                    of all 8 corners of a chunk of samples in LDS; every wave scans that list in order, 64 entries per
//                    step, and adds the entries that fall into its tile one after the other.  A cell of grad_value is
//                    therefore summed by ONE wave in ascending (query, level, point, corner) order whatever the launch
//                    shape is, rounded once and stored once: no atomics, no zero fill, the same bits on every run.
#include <cstdlib>
#include <type_traits>
#include "ver_common.h"

namespace {

constexpr int kMaxLP = 32, kMaxHd = 128, kMaxHeads = 64;
constexpr int kTileKeys = 16, kWaves = 4, kBlockKeys = kTileKeys * kWaves;   // k_dattn3d_bwd_v
constexpr int kChunkBytes = 30 * 1024;   // sample list + grad_out rows of one query chunk (beside <= 32 KiB of accumulators)

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float ld(const void* p, long i, int bf) {
    return bf ? bf16_to_f32(static_cast<const uint16_t*>(p)[i]) : static_cast<const float*>(p)[i];
}

__device__ __forceinline__ void st(void* p, long i, int bf, float v) {
    if (bf)
        static_cast<uint16_t*>(p)[i] = f32_to_bf16_rne(v);
    else
        static_cast<float*>(p)[i] = v;
}

// maximum and sum of exp(logit - maximum) of the LP logits that start at `base`
__device__ __forceinline__ void softmax_stats(const void* logits, long base, int LP, int qbf, float& m, float& s) {
    m = ld(logits, base, qbf);
    for (int i = 1; i < LP; ++i) m = fmaxf(m, ld(logits, base + i, qbf));
    s = 0.0f;
    for (int i = 0; i < LP; ++i) s += expf(ld(logits, base + i, qbf) - m);
}

__device__ __forceinline__ float softmax_weight(const void* logits, long i, int qbf, float m, float s) {
    return expf(ld(logits, i, qbf) - m) / s;
}

// loc = ref + offset / (W, H, D): the division first, then the add, as the torch chain orders them
__device__ __forceinline__ void sample_loc(const float* __restrict__ r, const void* offsets, long o, int qbf, int D, int H,
                                           int W, float& x, float& y, float& z) {
    x = r[0] + ld(offsets, o, qbf) / (float)W;
    y = r[1] + ld(offsets, o + 1, qbf) / (float)H;
    z = r[2] + ld(offsets, o + 2, qbf) / (float)D;
}

template <bool VBF>
__device__ __forceinline__ float ldv(const void* p, long i) {
    if constexpr (VBF)
        return bf16_to_f32(static_cast<const uint16_t*>(p)[i]);
    else
        return static_cast<const float*>(p)[i];
}

}  // namespace

template <int G, int NC, bool VBF>
__global__ __launch_bounds__(256) void k_dattn3d_fwd(const void* __restrict__ value, const int64_t* __restrict__ shapes,
                                                     const int64_t* __restrict__ lstart, const float* __restrict__ ref,
                                                     const void* __restrict__ offsets, const void* __restrict__ logits,
                                                     void* __restrict__ out, int qbf, int obf, int B, int Nk, int heads,
                                                     int hd, int L, int P, int Nq) {
    const int gpb = 256 / G;
    const long gid = (long)blockIdx.x * gpb + threadIdx.x / G;
    const int lane = threadIdx.x % G;
    if (gid >= (long)B * Nq * heads) return;
    const int h = (int)(gid % heads);
    const long bq = gid / heads;
    const long b = bq / Nq;
    const int LP = L * P;
    const long sbase = gid * LP;
    const long vstride = (long)heads * hd;
    const long vb = b * Nk * vstride + (long)h * hd;
    float m, ssum;
    softmax_stats(logits, sbase, LP, qbf, m, ssum);
    float acc[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) acc[i] = 0.0f;
    for (int l = 0; l < L; ++l) {
        const int D = (int)shapes[3 * l], H = (int)shapes[3 * l + 1], W = (int)shapes[3 * l + 2];
        const long k0 = lstart[l];
        const float* r = ref + (bq * L + l) * 3;
        for (int p = 0; p < P; ++p) {
            float x, y, z;
            sample_loc(r, offsets, (sbase + l * P + p) * 3, qbf, D, H, W, x, y, z);
            Trilinear s;
            trilinear_setup<false>(x, y, z, D, H, W, s);
            if (!s.any) continue;
            const float a = softmax_weight(logits, sbase + l * P + p, qbf, m, ssum);
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const int ch = lane + i * G;
                if (ch < hd) {
                    float v = 0.0f;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        v += s.w[k] * ldv<VBF>(value, vb + min(k0 + s.key[k], (long)Nk - 1) * vstride + ch);
                    acc[i] += a * v;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int ch = lane + i * G;
        if (ch < hd) st(out, gid * hd + ch, obf, acc[i]);
    }
}

// LDS (floats): s_a [heads*LP] softmax weights, s_g [heads*LP] d(attention weight), s_gl [heads*LP*3] d(loc)
template <int G, int NC, bool VBF>
__global__ __launch_bounds__(256) void k_dattn3d_bwd_q(const void* __restrict__ value, const int64_t* __restrict__ shapes,
                                                       const int64_t* __restrict__ lstart, const float* __restrict__ ref,
                                                       const void* __restrict__ offsets, const void* __restrict__ logits,
                                                       const void* __restrict__ gout, void* __restrict__ goffsets,
                                                       void* __restrict__ glogits, float* __restrict__ gref, int qbf,
                                                       int obf, int Nk, int heads, int hd, int L, int P, int Nq) {
    extern __shared__ float sm[];
    const int LP = L * P;
    float* s_a = sm;
    float* s_g = sm + heads * LP;
    float* s_gl = sm + 2 * heads * LP;
    const long bq = blockIdx.x;
    const long b = bq / Nq;
    const int gpb = blockDim.x / G, grp = threadIdx.x / G, lane = threadIdx.x % G;
    const long vstride = (long)heads * hd;
    for (int h = grp; h < heads; h += gpb) {        // (no barrier in here: the groups' trip counts differ)
        const long gid = bq * heads + h;
        const long sbase = gid * LP;
        const long vb = b * Nk * vstride + (long)h * hd;
        float g[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int ch = lane + i * G;
            g[i] = ch < hd ? ld(gout, gid * hd + ch, obf) : 0.0f;
        }
        float m, ssum;
        softmax_stats(logits, sbase, LP, qbf, m, ssum);
        for (int l = 0; l < L; ++l) {
            const int D = (int)shapes[3 * l], H = (int)shapes[3 * l + 1], W = (int)shapes[3 * l + 2];
            const long k0 = lstart[l];
            const float* r = ref + (bq * L + l) * 3;
            for (int p = 0; p < P; ++p) {
                float x, y, z;
                sample_loc(r, offsets, (sbase + l * P + p) * 3, qbf, D, H, W, x, y, z);
                Trilinear s;
                trilinear_setup<true>(x, y, z, D, H, W, s);
                const float a = softmax_weight(logits, sbase + l * P + p, qbf, m, ssum);
                float sa = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
                if (s.any) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if (s.w[k] == 0.0f && s.gx[k] == 0.0f && s.gy[k] == 0.0f && s.gz[k] == 0.0f) continue;
                        float d = 0.0f;
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            const int ch = lane + i * G;
                            if (ch < hd) d += g[i] * ldv<VBF>(value, vb + min(k0 + s.key[k], (long)Nk - 1) * vstride + ch);
                        }
                        sa += s.w[k] * d;
                        sx += s.gx[k] * d;
                        sy += s.gy[k] * d;
                        sz += s.gz[k] * d;
                    }
                }
                sa = group_sum<G>(sa);
                sx = group_sum<G>(sx);
                sy = group_sum<G>(sy);
                sz = group_sum<G>(sz);
                if (lane == 0) {
                    const int o = h * LP + l * P + p;
                    s_a[o] = a;
                    s_g[o] = sa;
                    s_gl[o * 3] = (float)W * a * sx;
                    s_gl[o * 3 + 1] = (float)H * a * sy;
                    s_gl[o * 3 + 2] = (float)D * a * sz;
                }
            }
        }
    }
    __syncthreads();
    // softmax backward and d(offsets) = d(loc) / (W, H, D): one thread per (head, level, point)
    for (int t = threadIdx.x; t < heads * LP; t += blockDim.x) {
        const int h = t / LP, l = (t - h * LP) / P;
        float dot = 0.0f;
        for (int j = 0; j < LP; ++j) dot += s_a[h * LP + j] * s_g[h * LP + j];
        const long o = bq * heads * LP + t;
        st(glogits, o, qbf, s_a[t] * (s_g[t] - dot));
        const int D = (int)shapes[3 * l], H = (int)shapes[3 * l + 1], W = (int)shapes[3 * l + 2];
        st(goffsets, o * 3, qbf, s_gl[t * 3] / (float)W);
        st(goffsets, o * 3 + 1, qbf, s_gl[t * 3 + 1] / (float)H);
        st(goffsets, o * 3 + 2, qbf, s_gl[t * 3 + 2] / (float)D);
    }
    // d(ref[b, q, l, :]) = sum of d(loc) over the heads (ascending), then the points
    if (gref != nullptr) {
        for (int t = threadIdx.x; t < L * 3; t += blockDim.x) {
            const int l = t / 3, c = t - l * 3;
            float s = 0.0f;
            for (int h = 0; h < heads; ++h)
                for (int p = 0; p < P; ++p) s += s_gl[(h * LP + l * P + p) * 3 + c];
            gref[bq * L * 3 + t] = s;
        }
    }
}

// LDS: acc f32 [kWaves][kTileKeys][hd] | gs f32 [QC][hd] grad_out rows of the chunk | ent_coef f32 [QC*LP*8] | ent_key i32 [QC*LP*8]
__global__ __launch_bounds__(256) void k_dattn3d_bwd_v(const int64_t* __restrict__ shapes, const int64_t* __restrict__ lstart,
                                                       const float* __restrict__ ref, const void* __restrict__ offsets,
                                                       const void* __restrict__ logits, const void* __restrict__ gout,
                                                       void* __restrict__ gvalue, int vbf, int qbf, int obf, int Nk,
                                                       int heads, int hd, int L, int P, int Nq, int QC, int ktiles) {
    extern __shared__ float sm[];
    const int LP = L * P;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long bh = blockIdx.x / ktiles;
    const int kt = (int)(blockIdx.x - bh * ktiles);
    const long b = bh / heads;
    const int h = (int)(bh - b * heads);
    const int tile_base = kt * kBlockKeys + wave * kTileKeys;
    float* acc = sm + wave * kTileKeys * hd;
    float* gs = sm + kBlockKeys * hd;
    float* ent_coef = gs + QC * hd;
    int* ent_key = reinterpret_cast<int*>(ent_coef + QC * LP * 8);
    for (int i = tid; i < kBlockKeys * hd; i += 256) sm[i] = 0.0f;
    const float inv_lp = 1.0f / (float)LP;
    for (int q0 = 0; q0 < Nq; q0 += QC) {
        const int nq = min(QC, Nq - q0);
        const int ns = nq * LP;
        __syncthreads();        // the scans of the previous chunk are over (first pass: the accumulators are cleared)
        for (int i = tid; i < nq * hd; i += 256) {
            const int ql = i / hd, c = i - ql * hd;
            gs[i] = ld(gout, (((b * Nq + q0 + ql) * heads) + h) * hd + c, obf);
        }
        for (int s = tid; s < ns; s += 256) {
            const int ql = s / LP, i = s - ql * LP, l = i / P;
            const long bq = b * Nq + q0 + ql;
            const long sbase = (bq * heads + h) * LP;
            float m, ssum;
            softmax_stats(logits, sbase, LP, qbf, m, ssum);
            const float a = softmax_weight(logits, sbase + i, qbf, m, ssum);
            const int D = (int)shapes[3 * l], H = (int)shapes[3 * l + 1], W = (int)shapes[3 * l + 2];
            float x, y, z;
            sample_loc(ref + (bq * L + l) * 3, offsets, (sbase + i) * 3, qbf, D, H, W, x, y, z);
            Trilinear t;
            trilinear_setup<false>(x, y, z, D, H, W, t);
            const int k0 = (int)lstart[l];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ent_key[s * 8 + k] = t.w[k] != 0.0f ? k0 + t.key[k] : -1;     // -1: in no tile
                ent_coef[s * 8 + k] = a * t.w[k];
            }
        }
        __syncthreads();
        const int ne = ns * 8;
        for (int e0 = 0; e0 < ne; e0 += 64) {
            const int e = e0 + lane;
            const int key = e < ne ? ent_key[e] : -1;
            unsigned long long hits = __ballot((unsigned)(key - tile_base) < (unsigned)kTileKeys);
            while (hits) {                                  // ascending entry order: the order of the sum
                const int ee = e0 + __ffsll(hits) - 1;
                hits &= hits - 1;
                const int row = ent_key[ee] - tile_base;
                const float cf = ent_coef[ee];
                const int ql = (int)(((float)(ee >> 3) + 0.5f) * inv_lp);      // (ee / 8) / LP, exact below 2^16 samples
                for (int c = lane; c < hd; c += 64) acc[row * hd + c] += cf * gs[ql * hd + c];
            }
        }
    }
    // every lane reads back the cells it accumulated itself
    for (int r = 0; r < kTileKeys; ++r) {
        const int key = tile_base + r;
        if (key >= Nk) break;
        for (int c = lane; c < hd; c += 64) st(gvalue, ((b * Nk + key) * heads + h) * hd + c, vbf, acc[r * hd + c]);
    }
}

namespace {

template <typename F>
int dispatch_group(int hd, F&& f) {
    if (hd <= 8) return f(std::integral_constant<int, 8>(), std::integral_constant<int, 1>());
    if (hd <= 16) return f(std::integral_constant<int, 16>(), std::integral_constant<int, 1>());
    if (hd <= 32) return f(std::integral_constant<int, 32>(), std::integral_constant<int, 1>());
    if (hd <= 64) return f(std::integral_constant<int, 64>(), std::integral_constant<int, 1>());
    if (hd <= 96) return f(std::integral_constant<int, 32>(), std::integral_constant<int, 3>());
    return f(std::integral_constant<int, 64>(), std::integral_constant<int, 2>());
}

int group_lanes(int hd) {
    return dispatch_group(hd, [](auto g, auto) { return (int)decltype(g)::value; });
}

int chunk_queries(int hd, int LP, int Nq) {
    const int per_query = LP * 8 * 8 + hd * 4;
    const int qc = kChunkBytes / per_query;                // >= 12 (levels * points <= 32, head_dim <= 128)
    const int chunks = (Nq + qc - 1) / qc;                 // equal chunks: 100 decoder queries are 34 + 34 + 32, not 48 + 48 + 4
    return (Nq + chunks - 1) / chunks;
}

long key_tiles(int Nk) { return ((long)Nk + kBlockKeys - 1) / kBlockKeys; }

const char* range_error(int B, int Nk, int heads, int hd, int L, int P, int Nq) {
    if ((long)L * P > kMaxLP) return "levels * points > 32";
    if (hd > kMaxHd) return "head_dim > 128";
    if (heads > kMaxHeads) return "heads > 64";
    const long lim = 1L << 31;
    if ((long)B * Nq * heads >= lim || (long)B * heads * key_tiles(Nk) >= lim) return "more than 2^31 workgroups";
    return nullptr;
}

int check_sizes(const char* what, int vdt, int qdt, int odt, int B, int Nk, int heads, int hd, int L, int P, int Nq) {
    VER_REQUIRE(B >= 0 && Nq >= 0, VER_EINVAL, "%s: negative batch/query count", what);
    VER_REQUIRE(Nk > 0 && heads > 0 && hd > 0 && L > 0 && P > 0, VER_EINVAL,
                "%s: num_keys/heads/head_dim/levels/points must be positive", what);
    VER_REQUIRE((vdt == 0 || vdt == 1) && (qdt == 0 || qdt == 1) && (odt == 0 || odt == 1), VER_EINVAL,
                "%s: value_dtype/q_dtype/out_dtype must be 0 (f32) or 1 (bf16)", what);
    return VER_OK;
}

}  // namespace

extern "C" int ver_dattn3d_supported(int B, int num_keys, int heads, int head_dim, int levels, int points, int Nq) {
    if (B < 0 || Nq < 0 || num_keys <= 0 || heads <= 0 || head_dim <= 0 || levels <= 0 || points <= 0) return 0;
    return range_error(B, num_keys, heads, head_dim, levels, points, Nq) == nullptr ? 1 : 0;
}

extern "C" int ver_dattn3d_forward(const void* value, int value_dtype, const int64_t* shapes_dhw,
                                   const int64_t* level_start, const float* ref, const void* offsets, const void* logits,
                                   int q_dtype, void* out, int out_dtype, int B, int num_keys, int heads, int head_dim,
                                   int levels, int points, int Nq, void* stream) {
    int rc = check_sizes("ver_dattn3d_forward", value_dtype, q_dtype, out_dtype, B, num_keys, heads, head_dim, levels, points,
                         Nq);
    if (rc) return rc;
    if (B == 0 || Nq == 0) return VER_OK;
    VER_REQUIRE(value && shapes_dhw && level_start && ref && offsets && logits && out, VER_EINVAL,
                "ver_dattn3d_forward: null pointer argument");
    const char* why = range_error(B, num_keys, heads, head_dim, levels, points, Nq);
    VER_REQUIRE(why == nullptr, VER_EUNSUPPORTED, "ver_dattn3d_forward: %s (B %d, keys %d, heads %d, head_dim %d, levels %d, points %d, Nq %d)",
                why, B, num_keys, heads, head_dim, levels, points, Nq);
    const long total = (long)B * Nq * heads;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_group(head_dim, [&](auto g, auto nc) {
        constexpr int G = decltype(g)::value, NC = decltype(nc)::value;
        const int gpb = 256 / G;
        const dim3 grid((unsigned)((total + gpb - 1) / gpb));
        if (value_dtype)
            hipLaunchKernelGGL((k_dattn3d_fwd<G, NC, true>), grid, dim3(256), 0, st, value, shapes_dhw, level_start, ref,
                               offsets, logits, out, q_dtype, out_dtype, B, num_keys, heads, head_dim, levels, points, Nq);
        else
            hipLaunchKernelGGL((k_dattn3d_fwd<G, NC, false>), grid, dim3(256), 0, st, value, shapes_dhw, level_start, ref,
                               offsets, logits, out, q_dtype, out_dtype, B, num_keys, heads, head_dim, levels, points, Nq);
        return ver_check_launch("ver_dattn3d_forward");
    });
}

extern "C" int ver_dattn3d_backward(const void* value, int value_dtype, const int64_t* shapes_dhw,
                                    const int64_t* level_start, const float* ref, const void* offsets, const void* logits,
                                    int q_dtype, const void* grad_out, int out_dtype, void* grad_value, void* grad_offsets,
                                    void* grad_logits, float* grad_ref, int B, int num_keys, int heads, int head_dim,
                                    int levels, int points, int Nq, void* stream) {
    int rc = check_sizes("ver_dattn3d_backward", value_dtype, q_dtype, out_dtype, B, num_keys, heads, head_dim, levels,
                         points, Nq);
    if (rc) return rc;
    if (B == 0 || Nq == 0) return VER_OK;
    VER_REQUIRE(value && shapes_dhw && level_start && ref && offsets && logits && grad_out && grad_value && grad_offsets &&
                    grad_logits,
                VER_EINVAL, "ver_dattn3d_backward: null pointer argument");
    const char* why = range_error(B, num_keys, heads, head_dim, levels, points, Nq);
    VER_REQUIRE(why == nullptr, VER_EUNSUPPORTED, "ver_dattn3d_backward: %s (B %d, keys %d, heads %d, head_dim %d, levels %d, points %d, Nq %d)",
                why, B, num_keys, heads, head_dim, levels, points, Nq);
    hipStream_t st = (hipStream_t)stream;
    const int LP = levels * points;
    rc = dispatch_group(head_dim, [&](auto g, auto nc) {
        constexpr int G = decltype(g)::value, NC = decltype(nc)::value;
        int threads = (heads * G + 63) / 64 * 64;
        if (threads > 256) threads = 256;
        const dim3 grid((unsigned)((long)B * Nq));
        const size_t lds = (size_t)heads * LP * 5 * sizeof(float);
        if (value_dtype)
            hipLaunchKernelGGL((k_dattn3d_bwd_q<G, NC, true>), grid, dim3(threads), lds, st, value, shapes_dhw, level_start,
                               ref, offsets, logits, grad_out, grad_offsets, grad_logits, grad_ref, q_dtype, out_dtype,
                               num_keys, heads, head_dim, levels, points, Nq);
        else
            hipLaunchKernelGGL((k_dattn3d_bwd_q<G, NC, false>), grid, dim3(threads), lds, st, value, shapes_dhw, level_start,
                               ref, offsets, logits, grad_out, grad_offsets, grad_logits, grad_ref, q_dtype, out_dtype,
                               num_keys, heads, head_dim, levels, points, Nq);
        return ver_check_launch("ver_dattn3d_backward (queries)");
    });
    if (rc) return rc;
    const int qc = chunk_queries(head_dim, LP, Nq);
    const long ktiles = key_tiles(num_keys);
    const size_t lds = ((size_t)kBlockKeys * head_dim + (size_t)qc * head_dim + (size_t)qc * LP * 16) * sizeof(float);
    hipLaunchKernelGGL(k_dattn3d_bwd_v, dim3((unsigned)((long)B * heads * ktiles)), dim3(256), lds, st, shapes_dhw,
                       level_start, ref, offsets, logits, grad_out, grad_value, value_dtype, q_dtype, out_dtype, num_keys,
                       heads, head_dim, levels, points, Nq, qc, (int)ktiles);
    return ver_check_launch("ver_dattn3d_backward (keys)");
}
