// Batched rectangular linear sum assignment (include/ver_ops.h: ver_lsa_solve): the Hungarian matching of the detection
// branch's targets, scipy.optimize.linear_sum_assignment on every [R, ncols[p]] cost matrix of a batch, on the device.
//
// Algorithm: shortest augmenting paths (Jonker-Volgenant as restated by Crouse 2016, the form scipy implements), on the
// orientation with fewer "rows": one Dijkstra-like search over the columns per row, then the dual update and the flip of the
// augmenting path.  u, v and the path costs are fp64 as in scipy, and every expression is evaluated in scipy's order
// (((minVal + c) - u[i]) - v[j]), so with fp32 inputs the same comparisons come out the same way; only the choice among
// EQUAL path costs differs (scipy's follows the order of its shrinking work list): here the smallest cost wins, among equals
// an unassigned column, among those the lowest index.
//
// Mapping: ONE WAVEFRONT PER PROBLEM (a 64-thread workgroup).  A problem is a few hundred strictly sequential search steps of
// one pass over <= 1024 columns each -- latency, not bandwidth -- and the L * bs problems of a step are independent: that is
// the parallelism.  The columns are strided over the 64 lanes, the arg-min of a step is a 6-stage butterfly over
// (cost, key), the search state (v, path costs, path, the two matchings, the visited flags, u) sits in LDS: 28 bytes per
// column + 12 per row, 40 KiB at the 1024 x 1024 bound, 4 KiB at the 100 queries of vocc.py.  The cost matrix is read in
// place through L2 (one element per column and step; 8 KiB per problem at 100 x 20, read once in full by the validity scan
// that precedes the search).  The workgroup is one wave, so __syncthreads() below is no hardware barrier: it only orders the
// LDS traffic of the lanes for the compiler.
#include <climits>
#include <cmath>
#include "ver_common.h"

namespace {

constexpr int kLsaMax = 1024;          // supported R and Ccap
constexpr int kAssignedBit = 1 << 20;  // tie key = (column already assigned ? kAssignedBit : 0) | column  (column < 2^20)

__global__ __launch_bounds__(VER_WAVE) void k_lsa_solve(const float* __restrict__ cost, const int* __restrict__ ncols,
                                                        int* __restrict__ match, int* __restrict__ bad, int R, int Ccap, int NL,
                                                        int NS) {
    extern __shared__ double lsa_smem[];
    double* v = lsa_smem;           // [NL] dual of the long side
    double* shortest = v + NL;      // [NL] path cost of this search
    double* u = shortest + NL;      // [NS] dual of the short side
    int* path = reinterpret_cast<int*>(u + NS);   // [NL] short-side predecessor on the shortest path
    int* row4col = path + NL;       // [NL] short-side partner of a long-side index, -1
    int* visited = row4col + NL;    // [NL] scipy's SC
    int* col4row = visited + NL;    // [NS] long-side partner of a short-side index, -1

    const int lane = threadIdx.x;
    const size_t p = blockIdx.x;
    const float* c = cost + p * (size_t)R * Ccap;
    int* m = match + p * (size_t)R;
    int nc = ncols[p];
    bool isbad = nc < 0 || nc > Ccap;            // (outside the declared range: nothing of the matrix is read)
    if (isbad) nc = 0;

    // scipy raises on a NaN or -inf ANYWHERE in the matrix, visited by the search or not: one pass over the valid entries
    const int total = R * nc;
#pragma unroll 4
    for (int idx = lane; idx < total; idx += VER_WAVE) {
        const int r = idx / nc;
        const float x = c[(size_t)r * Ccap + (idx - r * nc)];
        isbad |= (x != x) || x == -INFINITY;
    }
    isbad = __any(isbad);

    const bool transposed = nc < R;              // scipy: work on the transpose when there are fewer columns than rows
    const int ns = transposed ? nc : R, nl = transposed ? R : nc;
    const size_t stride_s = transposed ? 1 : Ccap, stride_l = transposed ? Ccap : 1;   // cost(i, j) = c[i * stride_s + j * stride_l]

    if (!isbad && ns > 0) {
        for (int j = lane; j < nl; j += VER_WAVE) {
            v[j] = 0.0;
            row4col[j] = -1;
        }
        for (int i = lane; i < ns; i += VER_WAVE) {
            u[i] = 0.0;
            col4row[i] = -1;
        }
        for (int cur = 0; cur < ns && !isbad; ++cur) {
            for (int j = lane; j < nl; j += VER_WAVE) {
                shortest[j] = INFINITY;
                visited[j] = 0;
            }
            __syncthreads();
            double min_val = 0.0;
            int i = cur, sink = -1;
            while (sink < 0) {
                const double ui = u[i];
                const float* ci = c + (size_t)i * stride_s;
                double best = INFINITY;
                int bkey = INT_MAX;
                for (int j = lane; j < nl; j += VER_WAVE) {
                    if (visited[j]) continue;
                    const double r = ((min_val + (double)ci[(size_t)j * stride_l]) - ui) - v[j];
                    double s = shortest[j];
                    if (r < s) {
                        s = r;
                        shortest[j] = r;
                        path[j] = i;
                    }
                    const int key = (row4col[j] >= 0 ? kAssignedBit : 0) | j;
                    if (s < best || (s == best && key < bkey)) {
                        best = s;
                        bkey = key;
                    }
                }
#pragma unroll
                for (int off = VER_WAVE / 2; off > 0; off >>= 1) {
                    const double ob = __shfl_xor(best, off, VER_WAVE);
                    const int ok = __shfl_xor(bkey, off, VER_WAVE);
                    if (ob < best || (ob == best && ok < bkey)) {
                        best = ob;
                        bkey = ok;
                    }
                }
                if (best == INFINITY) {          // no finite assignment (scipy: "cost matrix is infeasible")
                    isbad = true;
                    break;
                }
                min_val = best;
                const int j = __builtin_amdgcn_readfirstlane(bkey) & (kAssignedBit - 1);
                if ((j & (VER_WAVE - 1)) == lane) visited[j] = 1;     // (its owner: the only lane that reads the flag)
                const int partner = row4col[j];
                if (partner < 0)
                    sink = j;
                else
                    i = partner;
            }
            if (isbad) break;
            // duals: every visited column j moves by d = minVal - shortest[j], and so does its partner row (scipy's loop over
            // SR reads shortest[col4row[i]]: the same number); the sink has d = 0 and no partner
            for (int j = lane; j < nl; j += VER_WAVE) {
                if (!visited[j]) continue;
                const double d = min_val - shortest[j];
                v[j] -= d;
                const int partner = row4col[j];
                if (partner >= 0) u[partner] += d;
            }
            if (lane == 0) u[cur] += min_val;
            __syncthreads();
            if (lane == 0) {                     // flip the augmenting path sink -> cur
                int j = sink;
                for (;;) {
                    const int pi = path[j];
                    row4col[j] = pi;
                    const int next = col4row[pi];
                    col4row[pi] = j;
                    j = next;
                    if (pi == cur) break;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (isbad || ns == 0) {
        for (int r = lane; r < R; r += VER_WAVE) m[r] = -1;
        if (isbad && bad && lane == 0) atomicOr(bad, 1);
        return;
    }
    const int* out = transposed ? row4col : col4row;    // transposed: the long side IS the rows
    for (int r = lane; r < R; r += VER_WAVE) m[r] = out[r];
}

}  // namespace

extern "C" int ver_lsa_solve(const float* cost, const int32_t* ncols, int32_t* match, int32_t* bad, int P, int R, int Ccap,
                             void* stream) {
    VER_REQUIRE(P >= 0 && R >= 1 && Ccap >= 0, VER_EINVAL, "ver_lsa_solve: bad sizes P=%d R=%d Ccap=%d", P, R, Ccap);
    VER_REQUIRE(R <= kLsaMax && Ccap <= kLsaMax, VER_EUNSUPPORTED, "ver_lsa_solve: R=%d Ccap=%d (built for at most %d each)", R,
                Ccap, kLsaMax);
    if (P == 0) return VER_OK;
    VER_REQUIRE((cost || Ccap == 0) && ncols && match, VER_EINVAL, "ver_lsa_solve: null pointer argument");
    const int NL = R > Ccap ? R : Ccap, NS = R > Ccap ? (Ccap > 0 ? Ccap : 1) : R;
    const size_t lds = (size_t)NL * (2 * sizeof(double) + 3 * sizeof(int)) + (size_t)NS * (sizeof(double) + sizeof(int));
    hipLaunchKernelGGL(k_lsa_solve, dim3((unsigned)P), dim3(VER_WAVE), lds, (hipStream_t)stream, cost, ncols, match, bad, R, Ccap,
                       NL, NS);
    return ver_check_launch("ver_lsa_solve");
}
