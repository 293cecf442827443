// d(W2) of k_occ_mlp_bwd_ws accumulated in step 5 instead of step 7 (-DVER_WS_DW2_STEP7=0), out of csrc/ver_occ_mlp.hip at
// commit bb307c3.  Round 6 moved it to step 7: "equal time then, the better balance once the row team got lighter"
// (docs/HISTORY.md R6-6, 25.4 -> 25.1 ms together with the d(x) stores); the source called it "the same time on the box that
// measured both".  Step 7 was 0.5 k cycles of a slot the row team needs 2 k for, step 5 (3.1 k) had the row team idle for
// 1.5 k.  Nothing builds this.
// ------------------------------------------------------------------------------------------------------------------
// The two feature-team steps as they stood with the switch (kWsDw2InStep7 = VER_WS_DW2_STEP7, default 1; the
// VER_WS_ABL_NOSUMS guards around the row sums are left out):
    auto f5 = [&](__bf16* T) {                                            // LN2 row sums, d(h1) = W2^T d(a2) -> T4
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 ada[OT];
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) {
                ada[ot] = ns_tr_frag(T + 3 * kWsTile, kNsLd, 32 * ks, f0 + 16 * ot, c, g);
                sb2[ot] = mfma(ada[ot], ones, sb2[ot]);
                const bf16x8 adz = ns_tr_frag(T + 2 * kWsTile, kNsLd, 32 * ks, f0 + 16 * ot, c, g);
                sbet2[ot] = mfma(adz, ones, sbet2[ot]);
                sgam2[ot] = mfma(adz, ns_tr_frag(T + kWsTile, kNsLd, 32 * ks, f0 + 16 * ot, c, g), sgam2[ot]);
            }
            if constexpr (!kWsDw2InStep7) {
#pragma unroll
                for (int kt = 0; kt < 8; ++kt) {
                    const bf16x8 b = ns_tr_frag(T, kNsLd, 32 * ks, 16 * kt, c, g);
#pragma unroll
                    for (int ot = 0; ot < OT; ++ot) dw2[ot][kt] = mfma(ada[ot], b, dw2[ot][kt]);
                    if (kt & 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        rows_product(T + 3 * kWsTile, T4, wb2, nullptr);
    };
    auto f7 = [&](__bf16* T) {                                            // LN1 row sums from T2, T1; d(W2) from T3, T0
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 ada[OT];
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) {
                if constexpr (kWsDw2InStep7) ada[ot] = ns_tr_frag(T + 3 * kWsTile, kNsLd, 32 * ks, f0 + 16 * ot, c, g);
                const bf16x8 adz = ns_tr_frag(T + 2 * kWsTile, kNsLd, 32 * ks, f0 + 16 * ot, c, g);
                sbet1[ot] = mfma(adz, ones, sbet1[ot]);
                sgam1[ot] = mfma(adz, ns_tr_frag(T + kWsTile, kNsLd, 32 * ks, f0 + 16 * ot, c, g), sgam1[ot]);
            }
            if constexpr (kWsDw2InStep7) {
#pragma unroll
                for (int kt = 0; kt < 8; ++kt) {
                    const bf16x8 b = ns_tr_frag(T, kNsLd, 32 * ks, 16 * kt, c, g);
#pragma unroll
                    for (int ot = 0; ot < OT; ++ot) dw2[ot][kt] = mfma(ada[ot], b, dw2[ot][kt]);
                    if (kt & 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };
