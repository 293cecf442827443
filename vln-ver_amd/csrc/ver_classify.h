// The occupancy classification rule (head:1505-1540, focal-loss branch), shared by every entry point that turns a row of
// logits into a class: ver_occ_predict / ver_occ_confusion (ver_post.hip) and the classifying epilogues of the fused MLP
// forward (ver_occ_mlp.hip: ver_occ_mlp_confusion / ver_occ_mlp_classes).  A prediction is the same function everywhere
// because it is THIS code everywhere:
//     p = sigmoid(logit) in fp32;  best = torch.argmax(p) -- the first of equal maxima, NaN counts as the maximum and the
//     first NaN wins;  the threshold is one more, LAST column: it wins only when strictly greater than p[best].
// Plain C++ apart from the sigmoid (device only): the comparison rules also compile for the host (tests).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VER_CLASSIFY_FN __host__ __device__ __forceinline__
#else
#define VER_CLASSIFY_FN inline
#endif

#if defined(__HIPCC__)
// fp32 sigmoid as one fixed sequence of correctly rounded operations around expf: no contraction, no fast division
__device__ __forceinline__ float ver_class_prob(float logit) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-logit))); }
#endif

// sequential step of the arg-max: does probability `p` of a LATER class replace the running best `pb`?
VER_CLASSIFY_FN bool ver_class_takes(float p, float pb) { return (p > pb) || (std::isnan(p) && !std::isnan(pb)); }

// merge of two partial arg-maxima, segment A holding LOWER class indices than segment B: true when B's result stands.
// The same predicate as the sequential step, and for the same reason: B's best only has to beat the best of everything
// before it, ties and a second NaN stay with the earlier class -- so any split of a row gives the sequential result.
VER_CLASSIFY_FN bool ver_class_merge_takes_b(float pa, float pb_b) { return ver_class_takes(pb_b, pa); }

VER_CLASSIFY_FN void ver_class_merge(int best_a, float pa, int best_b, float pb_b, int& best, float& pb) {
    const bool b = ver_class_merge_takes_b(pa, pb_b);
    best = b ? best_b : best_a;
    pb = b ? pb_b : pa;
}

// the threshold is the LAST column: it wins only when strictly greater than every class probability
VER_CLASSIFY_FN int threshold_class(int best, float pb, float thr, int C) { return (!std::isnan(pb) && thr > pb) ? C : best; }
