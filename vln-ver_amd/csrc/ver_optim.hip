// Gradient clipping by the global L2 norm + AdamW over a list of fp32 tensors, two launches per step
// (include/ver_ops.h: ver_clip_adamw_*).  The reference's step is mmcv's OptimizerHook(grad_clip=dict(max_norm=...)) in front
// of torch.optim.AdamW (projects/configs/verformer/vocc.py:268-274): `clip_grad_norm_` = a per-tensor norm pass, a norm of
// norms and a multiply pass over every gradient; AdamW = another pass over parameter, gradient and both moments.  Here:
//   k_sqnorm      : per chunk of `chunk` elements, sum of squares of the gradient -> partial[chunk index]   (one read of g)
//   k_clip_adamw  : every workgroup adds the partials up IN ORDER (deterministic), forms the clip factor
//                   clamp(max_norm / (norm + 1e-6), max = 1) (NaN handed on, as torch.clamp does) and updates its chunk: g' = g * factor (not written back),
//                   p *= 1 - lr * wd;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
//                   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)                 -- torch.optim.AdamW, amsgrad off
// 28 bytes per parameter in all (p, g, m, v read; p, m, v written) + 4 for the norm: the step's 158 M parameters are two
// streaming passes of 0.6 + 4.4 GB instead of 1.7 ms in four torch passes.
#include "ver_common.h"

namespace {
struct Chunk {
    int tensor;
    int first;            // first chunk of that tensor
};

__device__ __forceinline__ float block_sum(float v) {
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ float bf16_widen(unsigned short b) { return __uint_as_float((unsigned)b << 16); }

// fp32 -> bf16, one rounding to nearest-even; NaN -> the quiet NaN 0x7fc0, +-inf stay (c10::BFloat16's rule: pack_host in
// hipops.py is the host model)
__device__ __forceinline__ unsigned short bf16_round(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// Where k_sqnorm / k_clip_adamw read the gradient of tensor t from: `at(t, start)` -> a cursor with `wide()` (16-byte loads
// of four elements are legal), `v4(i)` (elements 4i .. 4i+3) and `el(i)`, all as fp32.  One kernel body per loader, so the
// order of every sum and the compiler's contractions are those of the fp32 pointer-table form.
struct TableGrads {              // row 1 of the [4][n] pointer table: fp32 tensors of any 4-byte alignment
    const float* const* table;
    int n;
    struct Cursor {
        const float* g;
        __device__ bool wide() const { return (reinterpret_cast<uintptr_t>(g) & 15) == 0; }
        __device__ float4 v4(long i) const { return reinterpret_cast<const float4*>(g)[i]; }
        __device__ float el(long i) const { return g[i]; }
    };
    __device__ Cursor at(int t, long start) const { return {table[n + t] + start}; }
};

// flat + offsets[t]: offsets are multiples of 8 elements, chunk starts multiples of 4, flat itself 16-byte aligned -- four
// elements are always one aligned load (16 bytes of fp32, 8 of bf16)
struct FlatGradsF32 {
    const float* flat;
    const long* offsets;
    struct Cursor {
        const float* g;
        __device__ bool wide() const { return true; }
        __device__ float4 v4(long i) const { return reinterpret_cast<const float4*>(g)[i]; }
        __device__ float el(long i) const { return g[i]; }
    };
    __device__ Cursor at(int t, long start) const { return {flat + offsets[t] + start}; }
};

struct FlatGradsBF16 {
    const unsigned short* flat;
    const long* offsets;
    struct Cursor {
        const unsigned short* g;
        __device__ bool wide() const { return true; }
        __device__ float4 v4(long i) const {
            const ushort4 q = reinterpret_cast<const ushort4*>(g)[i];
            return make_float4(bf16_widen(q.x), bf16_widen(q.y), bf16_widen(q.z), bf16_widen(q.w));
        }
        __device__ float el(long i) const { return bf16_widen(g[i]); }
    };
    __device__ Cursor at(int t, long start) const { return {flat + offsets[t] + start}; }
};
}  // namespace

// grads: one of the loaders above; sizes [n], chunk_tensor [n_chunks], chunk_index [n_chunks] (index of the chunk inside its
// tensor)
template <class Grads>
__global__ __launch_bounds__(256) void k_sqnorm(const Grads grads, const long* __restrict__ sizes,
                                                const int* __restrict__ chunk_tensor, const int* __restrict__ chunk_index,
                                                int chunk, float* __restrict__ partial, int* __restrict__ steps) {
    const int t = chunk_tensor[blockIdx.x];
    // per-tensor update counters kept on the device (ver_clip_adamw_step_tensors): the first chunk of a tensor counts this
    // update; k_clip_adamw, next on the stream, reads the new count for its bias corrections
    if (steps && chunk_index[blockIdx.x] == 0 && threadIdx.x == 0) steps[t] += 1;
    const long start = (long)chunk_index[blockIdx.x] * chunk;
    const long len = min((long)chunk, sizes[t] - start);
    const typename Grads::Cursor g = grads.at(t, start);
    float s = 0.f;
    if (g.wide()) {
        const long nv = len >> 2;
        for (long i = threadIdx.x; i < nv; i += 256) {
            const float4 q = g.v4(i);
            s += q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
        }
        for (long i = (nv << 2) + threadIdx.x; i < len; i += 256) {
            const float e = g.el(i);
            s += e * e;
        }
    } else {
        for (long i = threadIdx.x; i < len; i += 256) {
            const float e = g.el(i);
            s += e * e;
        }
    }
    s = block_sum(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// hyper (or NULL: the scalar arguments hold for every tensor): [n][6] floats per tensor = lr, beta1, beta2, eps, weight decay,
// (unused); steps (with hyper): the number of updates of tensor t INCLUDING this one (k_sqnorm has counted it).  table: [4][n]
// device pointers (p | g | m | v); the gradient comes through `grads`, which may or may not read row 1
template <class Grads>
__global__ __launch_bounds__(256) void k_clip_adamw(const Grads grads, float* const* __restrict__ table, const long* __restrict__ sizes,
                                                    const int* __restrict__ chunk_tensor, const int* __restrict__ chunk_index,
                                                    int n, int chunk, const float* __restrict__ partial, int n_chunks,
                                                    float max_norm, float lr, float beta1, float beta2, float eps, float decay,
                                                    float step_size, float inv_sqrt_bc2, float* __restrict__ norm_out,
                                                    const float* __restrict__ hyper, const int* __restrict__ steps) {
    // the same in-order sum in every workgroup: no second launch, no atomics, a bitwise reproducible clip factor
    float s = 0.f;
    for (int i = threadIdx.x; i < n_chunks; i += 256) s += partial[i];
    s = block_sum(s);
    const float norm = sqrtf(s);
    // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to <= 1 by torch.clamp, which hands a NaN
    // on -- a non-finite norm poisons EVERY gradient (and with it every parameter), it does not leave the finite ones unclipped
    float factor = 1.0f;
    if (max_norm > 0.f) {
        const float coef = max_norm / (norm + 1e-6f);
        factor = coef < 1.0f ? coef : (coef != coef ? coef : 1.0f);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = norm;
    const int t = chunk_tensor[blockIdx.x];
    const long start = (long)chunk_index[blockIdx.x] * chunk;
    const long len = min((long)chunk, sizes[t] - start);
    float* p = table[t] + start;
    const typename Grads::Cursor g = grads.at(t, start);
    float* m = table[2 * n + t] + start;
    float* v = table[3 * n + t] + start;
    if (hyper) {
        const float* h = hyper + 6 * t;
        const double st = (double)steps[t];
        lr = h[0], beta1 = h[1], beta2 = h[2], eps = h[3];
        decay = (float)(1.0 - (double)lr * (double)h[4]);
        step_size = (float)((double)lr / (1.0 - pow((double)beta1, st)));
        inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, st)));
    }
    auto upd = [&](float& pp, float gg, float& mm, float& vv) {
        gg *= factor;
        pp *= decay;
        mm = beta1 * mm + (1.f - beta1) * gg;
        vv = beta2 * vv + (1.f - beta2) * gg * gg;
        pp -= step_size * mm / (sqrtf(vv) * inv_sqrt_bc2 + eps);
    };
    const bool vec = g.wide() && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) |
                                   reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    long done = 0;
    if (vec) {
        const long nv = len >> 2;
        for (long i = threadIdx.x; i < nv; i += 256) {
            float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
            const float4 gg = g.v4(i);
            upd(pp.x, gg.x, mm.x, vv.x), upd(pp.y, gg.y, mm.y, vv.y), upd(pp.z, gg.z, mm.z, vv.z), upd(pp.w, gg.w, mm.w, vv.w);
            reinterpret_cast<float4*>(p)[i] = pp, reinterpret_cast<float4*>(m)[i] = mm, reinterpret_cast<float4*>(v)[i] = vv;
        }
        done = nv << 2;
    }
    for (long i = done + threadIdx.x; i < len; i += 256) {
        float pp = p[i], mm = m[i], vv = v[i];
        upd(pp, g.el(i), mm, vv);
        p[i] = pp, m[i] = mm, v[i] = vv;
    }
}

extern "C" int ver_clip_adamw_step(void* const* table, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                                   int n_tensors, int n_chunks, int chunk_elems, float* partial, float* norm_out,
                                   float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                                   long step, void* stream) {
    VER_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && chunk_elems > 0 && chunk_elems % 4 == 0, VER_EINVAL,
                "ver_clip_adamw_step: bad sizes (%d tensors, %d chunks of %d)", n_tensors, n_chunks, chunk_elems);
    VER_REQUIRE(step >= 1, VER_EINVAL, "ver_clip_adamw_step: step %ld (the first update is step 1)", step);
    VER_REQUIRE(lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && weight_decay >= 0.f,
                VER_EINVAL, "ver_clip_adamw_step: hyper-parameters out of range");
    if (n_tensors == 0 || n_chunks == 0) return VER_OK;
    VER_REQUIRE(table && sizes && chunk_tensor && chunk_index && partial, VER_EINVAL, "ver_clip_adamw_step: null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    const TableGrads grads{(const float* const*)table, n_tensors};
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(k_sqnorm<TableGrads>, dim3(n_chunks), dim3(256), 0, st, grads, sizes, chunk_tensor, chunk_index,
                       chunk_elems, partial, (int*)nullptr);
    hipLaunchKernelGGL(k_clip_adamw<TableGrads>, dim3(n_chunks), dim3(256), 0, st, grads, (float* const*)table, sizes, chunk_tensor, chunk_index,
                       n_tensors, chunk_elems, (const float*)partial, n_chunks, max_norm, lr, beta1, beta2, eps,
                       (float)(1.0 - (double)lr * (double)weight_decay), (float)((double)lr / bc1), (float)(1.0 / sqrt(bc2)), norm_out,
                       (const float*)nullptr, (const int*)nullptr);
    return ver_check_launch("ver_clip_adamw_step");
}

namespace {
// the per-tensor step over any gradient loader: ver_clip_adamw_step_tensors and ver_clip_adamw_step_flat differ in `grads` alone
template <class Grads>
int step_tensors(const char* who, const Grads grads, void* const* table, const long* sizes, const int* chunk_tensor,
                 const int* chunk_index, const float* hyper, int* steps, int n_tensors, int n_chunks, int chunk_elems,
                 float* partial, float* norm_out, float max_norm, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sqnorm<Grads>, dim3(n_chunks), dim3(256), 0, st, grads, sizes, chunk_tensor, chunk_index, chunk_elems,
                       partial, steps);
    hipLaunchKernelGGL(k_clip_adamw<Grads>, dim3(n_chunks), dim3(256), 0, st, grads, (float* const*)table, sizes, chunk_tensor,
                       chunk_index, n_tensors, chunk_elems, (const float*)partial, n_chunks, max_norm, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f,
                       1.f, norm_out, hyper, (const int*)steps);
    return ver_check_launch(who);
}
}  // namespace

extern "C" int ver_clip_adamw_step_tensors(void* const* table, const long* sizes, const int* chunk_tensor, const int* chunk_index,
                                           const float* hyper, int* steps, int n_tensors, int n_chunks, int chunk_elems,
                                           float* partial, float* norm_out, float max_norm, void* stream) {
    VER_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && chunk_elems > 0 && chunk_elems % 4 == 0, VER_EINVAL,
                "ver_clip_adamw_step_tensors: bad sizes (%d tensors, %d chunks of %d)", n_tensors, n_chunks, chunk_elems);
    if (n_tensors == 0 || n_chunks == 0) return VER_OK;
    VER_REQUIRE(table && sizes && chunk_tensor && chunk_index && partial && hyper && steps, VER_EINVAL,
                "ver_clip_adamw_step_tensors: null pointer argument");
    return step_tensors("ver_clip_adamw_step_tensors", TableGrads{(const float* const*)table, n_tensors}, table, sizes, chunk_tensor,
                        chunk_index, hyper, steps, n_tensors, n_chunks, chunk_elems, partial, norm_out, max_norm, stream);
}

extern "C" int ver_clip_adamw_step_flat(void* const* table, const long* sizes, const long* offsets, const int* chunk_tensor,
                                        const int* chunk_index, const float* hyper, int* steps, const void* flat, int flat_dtype,
                                        int n_tensors, int n_chunks, int chunk_elems, float* partial, float* norm_out,
                                        float max_norm, void* stream) {
    const char* who = "ver_clip_adamw_step_flat";
    VER_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && chunk_elems > 0 && chunk_elems % 4 == 0, VER_EINVAL,
                "%s: bad sizes (%d tensors, %d chunks of %d)", who, n_tensors, n_chunks, chunk_elems);
    VER_REQUIRE(flat_dtype == VER_F32 || flat_dtype == VER_BF16, VER_EINVAL, "%s: flat_dtype %d (VER_F32 or VER_BF16)", who, flat_dtype);
    if (n_tensors == 0 || n_chunks == 0) return VER_OK;
    VER_REQUIRE(table && sizes && offsets && chunk_tensor && chunk_index && partial && hyper && steps && flat, VER_EINVAL,
                "%s: null pointer argument", who);
    VER_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 15) == 0, VER_EINVAL, "%s: flat must be 16-byte aligned", who);
    if (flat_dtype == VER_F32)
        return step_tensors(who, FlatGradsF32{(const float*)flat, offsets}, table, sizes, chunk_tensor, chunk_index, hyper, steps,
                            n_tensors, n_chunks, chunk_elems, partial, norm_out, max_norm, stream);
    return step_tensors(who, FlatGradsBF16{(const unsigned short*)flat, offsets}, table, sizes, chunk_tensor, chunk_index, hyper,
                        steps, n_tensors, n_chunks, chunk_elems, partial, norm_out, max_norm, stream);
}

// ver_grad_pack: flat[offsets[t] + i] = g_t[i] * scale, one workgroup per chunk of the optimizer's chunk tables.  A streaming
// copy (4 bytes read, 4 or 2 written per element): every lane moves 16 bytes per store -- one float4 load for an fp32 wire, two
// for eight bf16 -- when the gradient and the destination of the chunk are both 16-byte aligned; a gradient that is a view 4 or
// 8 bytes off (a bucket view) goes element by element, as in k_sqnorm.  Elements between the tensors are not touched.
template <class T> struct Wire;
template <> struct Wire<float> {
    static constexpr int W = 4;
    __device__ static float one(float f) { return f; }
    __device__ static void store(float* dst, long i, const float* g, float scale) {
        const float4 q = reinterpret_cast<const float4*>(g)[i];
        reinterpret_cast<float4*>(dst)[i] = make_float4(q.x * scale, q.y * scale, q.z * scale, q.w * scale);
    }
};
template <> struct Wire<unsigned short> {
    static constexpr int W = 8;
    __device__ static unsigned short one(float f) { return bf16_round(f); }
    __device__ static void store(unsigned short* dst, long i, const float* g, float scale) {
        const float4 a = reinterpret_cast<const float4*>(g)[2 * i], b = reinterpret_cast<const float4*>(g)[2 * i + 1];
        auto two = [&](float lo, float hi) { return (unsigned)bf16_round(lo * scale) | ((unsigned)bf16_round(hi * scale) << 16); };
        reinterpret_cast<uint4*>(dst)[i] = make_uint4(two(a.x, a.y), two(a.z, a.w), two(b.x, b.y), two(b.z, b.w));
    }
};

template <class T>
__global__ __launch_bounds__(256) void k_grad_pack(const float* const* __restrict__ table, const long* __restrict__ sizes,
                                                   const long* __restrict__ offsets, const int* __restrict__ chunk_tensor,
                                                   const int* __restrict__ chunk_index, int chunk, float scale, T* __restrict__ flat) {
    const int t = chunk_tensor[blockIdx.x];
    const long start = (long)chunk_index[blockIdx.x] * chunk;
    const long len = min((long)chunk, sizes[t] - start);
    const float* g = table[t] + start;
    T* dst = flat + offsets[t] + start;
    long done = 0;
    if (((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const long nv = len / Wire<T>::W;
        for (long i = threadIdx.x; i < nv; i += 256) Wire<T>::store(dst, i, g, scale);
        done = nv * Wire<T>::W;
    }
    for (long i = done + threadIdx.x; i < len; i += 256) dst[i] = Wire<T>::one(g[i] * scale);
}

extern "C" int ver_grad_pack(const void* const* table, const long* sizes, const long* offsets, const int* chunk_tensor,
                             const int* chunk_index, int n_tensors, int n_chunks, int chunk_elems, float scale, void* flat,
                             int flat_dtype, void* stream) {
    VER_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && chunk_elems > 0 && chunk_elems % 4 == 0, VER_EINVAL,
                "ver_grad_pack: bad sizes (%d tensors, %d chunks of %d)", n_tensors, n_chunks, chunk_elems);
    VER_REQUIRE(flat_dtype == VER_F32 || flat_dtype == VER_BF16, VER_EINVAL, "ver_grad_pack: flat_dtype %d (VER_F32 or VER_BF16)", flat_dtype);
    if (n_tensors == 0 || n_chunks == 0) return VER_OK;
    VER_REQUIRE(table && sizes && offsets && chunk_tensor && chunk_index && flat, VER_EINVAL, "ver_grad_pack: null pointer argument");
    VER_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 15) == 0, VER_EINVAL, "ver_grad_pack: flat must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (flat_dtype == VER_F32)
        hipLaunchKernelGGL(k_grad_pack<float>, dim3(n_chunks), dim3(256), 0, st, (const float* const*)table, sizes, offsets,
                           chunk_tensor, chunk_index, chunk_elems, scale, (float*)flat);
    else
        hipLaunchKernelGGL(k_grad_pack<unsigned short>, dim3(n_chunks), dim3(256), 0, st, (const float* const*)table, sizes, offsets,
                           chunk_tensor, chunk_index, chunk_elems, scale, (unsigned short*)flat);
    return ver_check_launch("ver_grad_pack");
}
