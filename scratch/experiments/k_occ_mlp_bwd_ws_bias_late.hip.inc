// The 64-row product of k_occ_mlp_bwd_ws (steps 1 and 5) with the bias b2 ADDED TO THE FINISHED TILE instead of being the
// accumulators' start value (-DVER_WS_BIAS_LATE=1), and with its ring depth as a -D knob (-DVER_WS_AHEAD=n), out of
// csrc/ver_occ_mlp.hip at commit bb307c3.  Round 6 (docs/HISTORY.md R6-6): requested at k-step 0 and added at k-step 3 the
// bias has four k-steps to arrive, but it stays live beside the accumulators (8 more registers); it was part of the fully
// pipelined form (a tile's four fragments ahead), which compiles as written and spills accumulators to scratch inside the round:
// 24.1 -> 31.4 ms.  What ships: the bias as the start value, two fragments ahead (a ring of three): 24.1 -> 23.1 ms.
// Nothing builds this.
// ------------------------------------------------------------------------------------------------------------------
// constexpr bool kWsBiasLate = VER_WS_BIAS_LATE;   // default 0
// constexpr int kWsAhead = VER_WS_AHEAD;           // default 2
    auto rows_product = [&](const __bf16* src, __bf16* dst, const bf16x8 (&w)[OT][4], const float* init) {
        constexpr int NF = 4 * RT, RING = kWsAhead + 1;
        bf16x8 b[RING];
        auto frag = [&](int i) { return *reinterpret_cast<const bf16x8*>(src + (16 * (i >> 2) + c) * kNsLd + 32 * (i & 3) + 8 * g); };
#pragma unroll
        for (int i = 0; i < kWsAhead; ++i) b[i] = frag(i);
        f32x4 acc[OT], bias[OT];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int rt = i >> 2, ks = i & 3;
            if (i + kWsAhead < NF) b[(i + kWsAhead) % RING] = frag(i + kWsAhead);
            if (ks == 0 && init) {
#pragma unroll
                for (int ot = 0; ot < OT; ++ot) bias[ot] = *reinterpret_cast<const f32x4*>(init + 16 * ot);
            }
            __builtin_amdgcn_sched_barrier(0);
            const bool late = kWsBiasLate || !init;
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) acc[ot] = mfma(w[ot][ks], b[i % RING], ks == 0 ? (late ? zero4 : bias[ot]) : acc[ot]);
            if (ks == 3) {
#pragma unroll
                for (int ot = 0; ot < OT; ++ot)
                    *reinterpret_cast<bf16x4*>(dst + (16 * rt + c) * kNsLd + f0 + 16 * ot + 4 * g) =
                        pack4(init && kWsBiasLate ? acc[ot] + bias[ot] : acc[ot]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
