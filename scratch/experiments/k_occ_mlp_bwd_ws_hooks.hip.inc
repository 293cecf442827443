// The measurement hooks of k_occ_mlp_bwd_ws that csrc/ver_occ_mlp.hip carried until commit bb307c3: three ablation builds
// (-DVER_WS_ABL_NOROW / _NOFEAT / _NOSUMS) and the fine timeline (-DVER_WS_TIMELINE_FINE, on top of -DVER_WS_TIMELINE, which
// stays).  Their numbers: profiles/r06_occ_mlp_bwd_timeline.txt, docs/HISTORY.md R5-MLP and R6-6.  Nothing builds this.
// ------------------------------------------------------------------------------------------------------------------
// VER_WS_ABL_NOROW: both row teams ran a round as eight barriers and nothing else --
//     for (int sl = 0; sl < 8; ++sl) lds_barrier();
// in place of the eight steps of the round loop (the feature team alone: 15.2 ms over 96.8 M rows).
// VER_WS_ABL_NOFEAT: the same in the feature team's round loop (the row team alone: 24.5 ms before round 6, 18.0 after).
// VER_WS_ABL_NOSUMS: f5 / f7 without the row-sum products sb2, sbet2, sgam2 / sbet1, sgam1 (28.5 ms against 29.9, mid-round).
//
// The fine timeline: four more stamps inside the LayerNorm backward (ln_bwd4) of the saved-statistics row team; they cost
// those steps ~600 cycles.  scratch/r06/ws_timeline.py reads them when the library exports ver_ws_timeline_fine_read.
__device__ long long g_ws_tl_fine[kWsTlProbes * 8 * kWsTlRounds * 8];
#define WS_TLF(k, idx)                                                                                              \
    do {                                                                                                            \
        const int pr_ = ws_tl_probe();                                                                              \
        const long kk_ = (k) - kWsTlFirst;                                                                          \
        if (pr_ >= 0 && kk_ >= 0 && kk_ < kWsTlRounds && (threadIdx.x & 63) == 0 && (idx) < 8)                      \
            g_ws_tl_fine[((pr_ * 8 + (threadIdx.x >> 6)) * kWsTlRounds + kk_) * 8 + (idx)] =                        \
                (long long)__builtin_amdgcn_s_memtime();                                                            \
    } while (0)
extern "C" int ver_ws_timeline_fine_read(long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ws_tl_fine), sizeof(long long) * kWsTlProbes * 8 * kWsTlRounds * 8);
}
// In the row team: `long tl_k = 0; int tl_base = 0;` in front of ln_bwd4, which stamped
//     WS_TLF(tl_k, tl_base + 0)   on entry
//     WS_TLF(tl_k, tl_base + 1)   behind the ReLU mask, the d(z) / n stores and the in-lane sums
//     WS_TLF(tl_k, tl_base + 2)   behind the eight group_sum<16>
//     WS_TLF(tl_k, tl_base + 3)   behind the last put()
// and the round loop set `tl_k = k; tl_base = 4;` behind slot 0 (B's step 6 in slot 1: stamps 4-7), `tl_base = 0;` behind
// slot 3 (A's step 4 in slot 4: stamps 0-3) and `tl_base = 8;` (off: idx < 8) behind that step.
