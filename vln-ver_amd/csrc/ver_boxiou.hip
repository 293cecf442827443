// Rotated 3-D box IoU and the per-image half of the indoor detection protocol (include/ver_ops.h: ver_box3d_overlaps,
// ver_det_match): what mmdet3d's BaseInstance3DBoxes.overlaps (height overlap x rotated BEV intersection) and the matching
// loop of the reference's datasets/indoor_eval.py:54-143 compute, on the device.
//
// The BEV intersection has no clipped polygon.  With B as the axis-aligned rectangle R = [-hx, hx] x [-hy, hy] of its own frame
// and A's four corners q0..q3 (counter-clockwise) in that frame, Green's theorem on g(x, y) = [|y| <= hy] clamp(x, -hx, hx)
// (dg/dx is the indicator of R) gives
//     area(A ^ R) = sum over A's edges of  integral g dy  =  sum (yb - ya) * mean of clamp(x) over the piece of the edge
//                                                                            inside the band |y| <= hy,
// ya, yb = the edge's end ordinates clamped into the band.  Only A's edges are walked, every term is a continuous function of
// the corners (an edge lying ON R's boundary contributes the same from either side: there is no closed / open comparison to
// get right, identical boxes included), and everything is statically indexed: no per-thread vertex array, no scratch.  The
// mean of clamp(x) over a linear piece is a weighted average of its three parts (below -hx, inside, above hx) with
// non-negative weights, so it has no cancellation; the constant clamp(x of A's centre) is subtracted from it (the (yb - ya)
// sum to zero round the polygon), which keeps the terms at the size of the intersection rather than of hx.
//
// Mapping.  ver_box3d_overlaps: a 256-thread workgroup per 32 x 32 tile of one sample's matrix, the 64 boxes' terms
// (centre, half extents, precise sinf / cosf, z range, volume, validity) staged in LDS once, four pairs per thread.
// ver_det_match: ONE WORKGROUP PER SAMPLE (as ver_assign.hip is one wave per problem: the samples are the parallelism), box
// terms of all predictions and ground truths in LDS, the same-class pairs clipped into an LDS matrix [Pcap][Gcap | 1], one
// thread per prediction for the arg-max of its row, one thread per prediction for the O(Pcap) scan of the evaluation order.
#include <cmath>
#include "ver_common.h"

namespace {

constexpr int kBoxThreads = 256;
constexpr int kTile = 32;               // ver_box3d_overlaps: boxes of a tile per side
constexpr int kMatchMaxBoxes = 1024;    // ver_det_match: Pcap, Gcap
constexpr int kMatchMaxPairs = 16384;   // ver_det_match: Pcap * Gcap (64 KiB of LDS for the matrix)
constexpr int kMaxThresholds = 8;

struct BoxTerms {
    float cx, cy, hx, hy, c, s, z0, z1, vol;
    int ok;
};

struct Thresholds {
    float v[kMaxThresholds];
};

__device__ __forceinline__ BoxTerms box_terms(const float* __restrict__ b, bool present) {
    BoxTerms t;
    const float x = b[0], y = b[1], z = b[2], dx = b[3], dy = b[4], dz = b[5], yaw = b[6];
    const bool finite = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(dx) && isfinite(dy) && isfinite(dz) && isfinite(yaw);
    t.ok = present && finite && dx > 0.0f && dy > 0.0f && dz > 0.0f;
    const float a = t.ok ? yaw : 0.0f;
    t.cx = x;
    t.cy = y;
    t.hx = 0.5f * dx;
    t.hy = 0.5f * dy;
    t.c = cosf(a);
    t.s = sinf(a);
    t.z0 = z;
    t.z1 = z + dz;
    t.vol = dx * dy * dz;
    return t;
}

// integral of [|y| <= hy] (clamp(x, -hx, hx) - xr) dy along the edge (x0, y0) -> (x1, y1)
__device__ __forceinline__ float edge_term(float x0, float y0, float x1, float y1, float hx, float hy, float xr) {
    const float ya = fminf(fmaxf(y0, -hy), hy), yb = fminf(fmaxf(y1, -hy), hy);
    const float wy = yb - ya;
    if (wy == 0.0f) return 0.0f;                      // outside the band, or parallel to it
    const float dy = y1 - y0, dx = x1 - x0;           // (wy != 0: y0 != y1)
    const float xa = x0 + (ya - y0) / dy * dx, xb = x0 + (yb - y0) / dy * dx;
    const float lo = fminf(xa, xb), hi = fmaxf(xa, xb);
    const float m0 = fminf(fmaxf(-hx, lo), hi), m1 = fminf(fmaxf(hx, lo), hi);
    const float len = hi - lo;
    const float num = (m0 - lo) * (-hx) + (m1 - m0) * (0.5f * (m0 + m1)) + (hi - m1) * hx;
    const float mean = len > 0.0f ? num / len : fminf(fmaxf(lo, -hx), hx);
    return wy * (mean - xr);
}

__device__ __forceinline__ float bev_intersection(const BoxTerms& a, const BoxTerms& b) {
    const float dx = a.cx - b.cx, dy = a.cy - b.cy;
    const float ox = b.c * dx + b.s * dy, oy = b.c * dy - b.s * dx;            // A's centre in B's frame
    const float cr = a.c * b.c + a.s * b.s, sr = a.s * b.c - a.c * b.s;        // cos, sin of yaw_a - yaw_b
    // separating axis (B's two, then A's two): disjoint or touching rectangles give exactly 0, not the rounding of a sum of
    // terms that cancel
    const float acr = fabsf(cr), asr = fabsf(sr);
    const float px = a.c * dx + a.s * dy, py = a.c * dy - a.s * dx;            // minus B's centre in A's frame
    if (fabsf(ox) >= acr * a.hx + asr * a.hy + b.hx || fabsf(oy) >= asr * a.hx + acr * a.hy + b.hy ||
        fabsf(px) >= acr * b.hx + asr * b.hy + a.hx || fabsf(py) >= asr * b.hx + acr * b.hy + a.hy)
        return 0.0f;
    const float uxx = cr * a.hx, uxy = sr * a.hx, uyx = -sr * a.hy, uyy = cr * a.hy;
    const float q0x = ox + uxx + uyx, q0y = oy + uxy + uyy;                    // (+, +)
    const float q1x = ox - uxx + uyx, q1y = oy - uxy + uyy;                    // (-, +)
    const float q2x = ox - uxx - uyx, q2y = oy - uxy - uyy;                    // (-, -)
    const float q3x = ox + uxx - uyx, q3y = oy + uxy - uyy;                    // (+, -)
    const float xr = fminf(fmaxf(ox, -b.hx), b.hx);
    const float area = edge_term(q0x, q0y, q1x, q1y, b.hx, b.hy, xr) + edge_term(q1x, q1y, q2x, q2y, b.hx, b.hy, xr) +
                       edge_term(q2x, q2y, q3x, q3y, b.hx, b.hy, xr) + edge_term(q3x, q3y, q0x, q0y, b.hx, b.hy, xr);
    return fmaxf(area, 0.0f);
}

__device__ __forceinline__ float pair_iou(const BoxTerms& a, const BoxTerms& b) {
    if (!a.ok || !b.ok) return 0.0f;
    const float h = fminf(a.z1, b.z1) - fmaxf(a.z0, b.z0);
    if (!(h > 0.0f)) return 0.0f;
    const float o = bev_intersection(a, b) * h;
    const float iou = o / fmaxf(a.vol + b.vol - o, 1e-8f);
    return isfinite(iou) ? iou : 0.0f;                // (extents whose volume leaves the fp32 range)
}

__global__ __launch_bounds__(kBoxThreads) void k_box3d_overlaps(const float* __restrict__ a, const int* __restrict__ na,
                                                                const float* __restrict__ b, const int* __restrict__ nb,
                                                                float* __restrict__ iou, int Acap, int Bcap, int tiles_a,
                                                                int tiles_b) {
    __shared__ BoxTerms terms[2 * kTile];
    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int tb = (int)(blk % tiles_b), ta = (int)((blk / tiles_b) % tiles_a);
    const size_t s = blk / ((size_t)tiles_b * tiles_a);
    const int a0 = ta * kTile, b0 = tb * kTile;
    const int ca = na ? min(max(na[s], 0), Acap) : Acap, cb = nb ? min(max(nb[s], 0), Bcap) : Bcap;
    if (tid < 2 * kTile) {
        const bool is_b = tid >= kTile;
        const int i = (is_b ? b0 : a0) + (tid & (kTile - 1));
        const int cap = is_b ? Bcap : Acap, cnt = is_b ? cb : ca;
        const float* src = (is_b ? b : a) + (s * (size_t)cap + (size_t)min(i, cap - 1)) * 7;
        terms[tid] = box_terms(src, i < cnt);
    }
    __syncthreads();
    const int j = tid & (kTile - 1);
    if (b0 + j >= Bcap) return;
    const BoxTerms tb_terms = terms[kTile + j];
#pragma unroll
    for (int r = 0; r < kTile * kTile / kBoxThreads; ++r) {
        const int i = (tid >> 5) + r * (kBoxThreads / kTile);
        if (a0 + i < Acap) iou[(s * (size_t)Acap + (size_t)(a0 + i)) * Bcap + (b0 + j)] = pair_iou(terms[i], tb_terms);
    }
}

__global__ __launch_bounds__(kBoxThreads) void k_det_match(const float* __restrict__ pred_boxes, const int* __restrict__ pred_labels,
                                                           const float* __restrict__ pred_scores,
                                                           const uint8_t* __restrict__ pred_valid,
                                                           const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                           const int* __restrict__ ngt, Thresholds thr, int num_thresholds,
                                                           float* __restrict__ iou_max, int* __restrict__ gt_index,
                                                           uint8_t* __restrict__ tp_bits, unsigned long long* __restrict__ npos,
                                                           int num_classes, int Pcap, int Gcap, int pitch) {
    extern __shared__ float match_smem[];
    float* mat = match_smem;                                             // [Pcap][pitch]: IoU of a same-class pair, else -1
    BoxTerms* pt = reinterpret_cast<BoxTerms*>(mat + (size_t)Pcap * pitch);   // [Pcap]
    BoxTerms* gt = pt + Pcap;                                            // [Gcap]
    int* plab = reinterpret_cast<int*>(gt + Gcap);                       // [Pcap] label, -1: matches nothing
    int* glab = plab + Pcap;                                             // [Gcap] label, -1: neither counted nor matched
    float* best = reinterpret_cast<float*>(glab + Gcap);                 // [Pcap] iou_max
    int* bidx = reinterpret_cast<int*>(best + Pcap);                     // [Pcap] gt_index
    float* score = reinterpret_cast<float*>(bidx + Pcap);                // [Pcap]
    int* bits = reinterpret_cast<int*>(score + Pcap);                    // [Pcap] thresholds below iou_max

    const int tid = threadIdx.x;
    const size_t s = blockIdx.x;
    const int ng = min(max(ngt[s], 0), Gcap);
    for (int d = tid; d < Pcap; d += kBoxThreads) {
        const size_t at = s * (size_t)Pcap + d;
        const int lab = pred_labels[at];
        const bool live = pred_valid[at] != 0 && lab >= 0 && lab < num_classes;
        pt[d] = box_terms(pred_boxes + at * 7, live);
        plab[d] = live ? lab : -1;
        score[d] = pred_scores[at];
    }
    for (int j = tid; j < Gcap; j += kBoxThreads) {
        const size_t at = s * (size_t)Gcap + j;
        const int lab = gt_labels[at];
        const bool live = j < ng && lab >= 0 && lab < num_classes;
        gt[j] = box_terms(gt_boxes + at * 7, live);
        glab[j] = live ? lab : -1;
        if (live) atomicAdd(npos + lab, 1ULL);
    }
    __syncthreads();
    const int pairs = Pcap * Gcap;
    for (int idx = tid; idx < pairs; idx += kBoxThreads) {
        const int d = idx / Gcap, j = idx - d * Gcap;
        const bool same = plab[d] >= 0 && plab[d] == glab[j];
        mat[d * pitch + j] = same ? pair_iou(pt[d], gt[j]) : -1.0f;
    }
    __syncthreads();
    for (int d = tid; d < Pcap; d += kBoxThreads) {
        float bv = -INFINITY;
        int bj = -1;
        for (int j = 0; j < Gcap; ++j) {
            const float v = mat[d * pitch + j];
            if (v >= 0.0f && v > bv) {                                   // first of equal maxima; -1 = not a candidate
                bv = v;
                bj = j;
            }
        }
        if (bj < 0) bv = 0.0f;
        int m = 0;
        if (bj >= 0) {
#pragma unroll
            for (int t = 0; t < kMaxThresholds; ++t) m |= (t < num_thresholds && bv > thr.v[t]) ? 1 << t : 0;
        }
        best[d] = bv;
        bidx[d] = bj;
        bits[d] = m;
    }
    __syncthreads();
    for (int d = tid; d < Pcap; d += kBoxThreads) {
        const int bj = bidx[d], mine = bits[d];
        const float sc = score[d];
        int taken = 0;
        if (mine) {
            for (int e = 0; e < Pcap; ++e) {
                const float se = score[e];
                const bool before = se > sc || (se == sc && e < d);
                taken |= (bidx[e] == bj && before) ? bits[e] : 0;
            }
        }
        const size_t at = s * (size_t)Pcap + d;
        iou_max[at] = best[d];
        gt_index[at] = bj;
        tp_bits[at] = (uint8_t)(mine & ~taken);
    }
}

}  // namespace

extern "C" int ver_box3d_overlaps(const float* a, const int32_t* na, const float* b, const int32_t* nb, float* iou, int S,
                                  int Acap, int Bcap, void* stream) {
    VER_REQUIRE(S >= 0 && Acap >= 0 && Bcap >= 0, VER_EINVAL, "ver_box3d_overlaps: bad sizes S=%d Acap=%d Bcap=%d", S, Acap, Bcap);
    if (S == 0 || Acap == 0 || Bcap == 0) return VER_OK;
    VER_REQUIRE(a && b && iou, VER_EINVAL, "ver_box3d_overlaps: null pointer argument");
    const long tiles_a = (Acap + kTile - 1) / kTile, tiles_b = (Bcap + kTile - 1) / kTile;
    const long blocks = tiles_a * tiles_b * S;
    VER_REQUIRE(blocks <= 0x7fffffffL, VER_EUNSUPPORTED, "ver_box3d_overlaps: %ld tiles of 32 x 32 pairs (at most 2^31 - 1)", blocks);
    hipLaunchKernelGGL(k_box3d_overlaps, dim3((unsigned)blocks), dim3(kBoxThreads), 0, (hipStream_t)stream, a, na, b, nb, iou,
                       Acap, Bcap, (int)tiles_a, (int)tiles_b);
    return ver_check_launch("ver_box3d_overlaps");
}

extern "C" int ver_det_match(const float* pred_boxes, const int32_t* pred_labels, const float* pred_scores,
                             const uint8_t* pred_valid, const float* gt_boxes, const int32_t* gt_labels, const int32_t* ngt,
                             const float* thresholds, int num_thresholds, float* iou_max, int32_t* gt_index, uint8_t* tp_bits,
                             int64_t* npos, int num_classes, int S, int Pcap, int Gcap, void* stream) {
    VER_REQUIRE(S >= 0 && Pcap >= 1 && Gcap >= 0 && num_classes >= 1, VER_EINVAL,
                "ver_det_match: bad sizes S=%d Pcap=%d Gcap=%d num_classes=%d", S, Pcap, Gcap, num_classes);
    VER_REQUIRE(num_thresholds >= 1 && num_thresholds <= kMaxThresholds, VER_EINVAL,
                "ver_det_match: num_thresholds=%d (1..%d)", num_thresholds, kMaxThresholds);
    VER_REQUIRE(Pcap <= kMatchMaxBoxes && Gcap <= kMatchMaxBoxes && (long)Pcap * Gcap <= kMatchMaxPairs, VER_EUNSUPPORTED,
                "ver_det_match: Pcap=%d Gcap=%d (built for at most %d each and %d pairs)", Pcap, Gcap, kMatchMaxBoxes,
                kMatchMaxPairs);
    if (S == 0) return VER_OK;
    VER_REQUIRE(pred_boxes && pred_labels && pred_scores && pred_valid && (Gcap == 0 || (gt_boxes && gt_labels)) && ngt &&
                    thresholds && iou_max && gt_index && tp_bits && npos,
                VER_EINVAL, "ver_det_match: null pointer argument");
    Thresholds thr;
    for (int t = 0; t < kMaxThresholds; ++t) thr.v[t] = t < num_thresholds ? thresholds[t] : INFINITY;
    const int pitch = Gcap | 1;                                          // odd: a wave's rows start on distinct banks
    const size_t lds = (size_t)Pcap * pitch * sizeof(float) + (size_t)(Pcap + Gcap) * (sizeof(BoxTerms) + sizeof(int)) +
                       (size_t)Pcap * 4 * sizeof(int);
    if (lds > 64 * 1024) {
        if (int rc = ver_lds_limit("ver_det_match", reinterpret_cast<const void*>(k_det_match), lds)) return rc;
    }
    hipLaunchKernelGGL(k_det_match, dim3((unsigned)S), dim3(kBoxThreads), lds, (hipStream_t)stream, pred_boxes, pred_labels,
                       pred_scores, pred_valid, gt_boxes, gt_labels, ngt, thr, num_thresholds, iou_max, gt_index, tp_bits,
                       reinterpret_cast<unsigned long long*>(npos), num_classes, Pcap, Gcap, pitch);
    return ver_check_launch("ver_det_match");
}
