// gemm_epilogue.inc -- the per-tile epilogue of the GEMM engine's kernels, textually included at the point where a
// corpus tile's 128 x 64 accumulators of a wave are complete (gemm_filter_kernel in kernels_gemm.h, and
// gemm_bf16_filter_kernel in kernels_gemm_bf16.h): MODE 1 dumps the scores; MODE 3 (the split filter's seeder) writes the best
// score of every group of 32 rows; MODE 0 runs the fast reject against the
// list / chip-wide thresholds and, on a hit, the append path (topk_dev.h). Expects in scope: acc[4][2] (f32x16), tile,
// lane, w, wu, q0, N, KP, cap, R, MODE, the kind flags COS / U8 / L2K with invn, invq, iq_lane, scale, the LDS object s
// (cnt, thr), my_lists, errflag, gslots, gthr, kk, kmargin (the k rule of topk_dev.h), tg_next[2], dump, ld_dump, kEpiPubEvery (one admission in so many re-derives the chip-wide bound), and kEpiTgWait = a vmcnt count no larger than the
// number of VMEM ops the wave issues per tile (the thresholds were requested a whole tile ago) and no smaller than the ops
// it keeps in flight (or the wait drains its prefetches). Ends by clearing acc and re-requesting tg_next.
            // ---------------- epilogue for corpus tile `tile` ----------------
            const size_t tb = (size_t)tile * kBC;
            const int half = lane >> 5, C = lane & 31;
            if (MODE == 1) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const size_t q = q0 + 64 * w + 2 * C + ct;
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                        for (int g = 0; g < 16; ++g) {
                            const size_t i = tb + 4 * ((g & 3) + 8 * (g >> 2) + 4 * half) + rt;
                            float v = acc[rt][ct][g];
                            if (COS) v = v * invn[i] * invq[q];
                            if (U8) v = v * scale + invq[q];
                            dump[q * ld_dump + i] = v;
                        }
                }
            } else if (MODE == 3) {
                // the split filter's seeder (kernels_gemm_bf16.h): no threshold is loaded, no list touched. Per query column and row
                // tile rt the best of the 32 rows tb + 4 i + rt -- this lane's 16 values g and those of its half-lane partner
                // (i = (g & 3) + 8 (g >> 2) + 4 half) -- as an order key, to row 4 tile + rt of the [rows / 32][ld_dump] key matrix
                uint32_t* const gmax = reinterpret_cast<uint32_t*>(dump);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const size_t q = q0 + 64 * w + 2 * C + ct;
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) {
                        uint32_t best = 0;
#pragma unroll
                        for (int g = 0; g < 16; ++g) {
                            const uint32_t o = f32_ord(acc[rt][ct][g]);
                            best = best > o ? best : o;
                        }
                        const uint32_t other = (uint32_t)__shfl_xor((int)best, 32, 64);
                        best = best > other ? best : other;
                        if (half == 0) gmax[((size_t)tile * 4 + rt) * ld_dump + q] = best;
                    }
                }
            } else {
                // Threshold of each of this lane's two queries: the better of the list's own (KP-th best it holds)
                // and the chip-wide bound gthr[q] (topk_dev.h, global threshold slots).
                uint32_t thr[2];
                use_after<kEpiTgWait>(tg_next[0], tg_next[1]);  // requested a whole tile ago (or before the first K-step)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const uint32_t tl = __hip_atomic_load(&s.thr[64 * w + 2 * C + ct], __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_WAVEFRONT);
                    // chip-wide bound as read at the end of the previous tile's epilogue: one tile stale (a stale
                    // bound is only weaker), but its L2 round trip is no longer on this wave's critical path
                    thr[ct] = tl > tg_next[ct] ? tl : tg_next[ct];
                }
                // Fast reject. For a threshold that is a non-negative float (the normal case once a list has KP
                // entries), "some value >= thr in total order" == "max over RAW BIT PATTERNS compared as signed
                // ints >= raw(thr)": non-negative floats (and +NaN, the greatest) order like their bits and every
                // negative float is a negative int. One v_max per value, no key conversion, NaN-safe.
                // The maxima are kept per group of 16 consecutive corpus rows (gq: rows tb + 32 gq + 16 half + [0,16)), so that
                // a visit of the append path walks only the groups that hold a hit: 16 sites instead of 64 per query.
                // (The cosine / L2 kinds keep ONE maximum per query column: their norm registers leave no room for eight, and
                //  a spilled accumulator in the K-loop costs more than the longer visits.)
                constexpr int NG = (COS || L2K) ? 1 : 4;
                int32_t gbest[2][NG];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int gg = 0; gg < NG; ++gg) gbest[ct][gg] = INT32_MIN;
                const float iq[2] = {iq_lane[0], iq_lane[1]};
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {  // 16 consecutive corpus rows: tb + 4*(8*gq + 4*half) + [0,16)
                    const float4* p = reinterpret_cast<const float4*>(invn + tb + 4 * (8 * gq + 4 * half));
#pragma unroll
                    for (int g3 = 0; g3 < 4; ++g3) {
                        float sc[4] = {1.0f, 1.0f, 1.0f, 1.0f};  // 1/||v|| of corpus rows 4*(g3 + ...) + rt
                        if (COS || L2K) {
                            const float4 t = p[g3];
                            sc[0] = t.x; sc[1] = t.y; sc[2] = t.z; sc[3] = t.w;
                        }
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                            for (int rt = 0; rt < 4; ++rt) {
                                float v = acc[rt][ct][4 * gq + g3];
                                if (COS) {
                                    v = v * sc[rt] * iq[ct];
                                    acc[rt][ct][4 * gq + g3] = v;
                                }
                                if (U8) {
                                    v = v * scale + iq[ct];
                                    acc[rt][ct][4 * gq + g3] = v;
                                }
                                if (L2K) {
                                    v = (2.0f * v + iq[ct]) - sc[rt];
                                    acc[rt][ct][4 * gq + g3] = v;
                                }
                                const int32_t raw = (int32_t)__float_as_uint(v);
                                gbest[ct][gq * NG / 4] = gbest[ct][gq * NG / 4] > raw ? gbest[ct][gq * NG / 4] : raw;
                            }
                    }
                    // keep the scheduler from hoisting all 16 norm loads (64 registers) above the first use: with the
                    // 128 accumulators live that is what pushed the cosine / L2 instantiations into scratch
                    if (COS || L2K) __builtin_amdgcn_sched_barrier(0);
                }
                bool hit[2];
                int32_t thr_raw[2];  // raw bits of the (non-negative) threshold; INT32_MIN = "no usable bound": everything passes
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const bool nonneg_thr = (thr[ct] & 0x80000000u) != 0;  // ord of a non-negative float
                    thr_raw[ct] = nonneg_thr ? (int32_t)(thr[ct] & 0x7fffffffu) : INT32_MIN;
                    int32_t b = gbest[ct][0];
#pragma unroll
                    for (int gg = 1; gg < NG; ++gg) b = b > gbest[ct][gg] ? b : gbest[ct][gg];
                    hit[ct] = b >= thr_raw[ct];
                }
                if (MODE == 2) {
                    // collect: a site that clears its query's fixed threshold goes to that query's global list (rare, and the
                    // only vector-memory traffic of this epilogue besides the threshold reload)
                    if (__any(hit[0] || hit[1])) {
                        uint32_t* const clist = reinterpret_cast<uint32_t*>(lists);
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct) {
                            const size_t q = q0 + 64 * w + 2 * C + ct;
                            const float thr_f = ord_f32(thr[ct]);
#pragma unroll
                            for (int gq = 0; gq < 4; ++gq) {
                                const bool ghit = hit[ct] && gbest[ct][gq * NG / 4] >= thr_raw[ct];
                                if (!__any(ghit)) continue;
                                if (ghit) {
#pragma unroll
                                    for (int g3 = 0; g3 < 4; ++g3)
#pragma unroll
                                        for (int rt = 0; rt < 4; ++rt) {
                                            const int g = 4 * gq + g3;
                                            if (acc[rt][ct][g] < thr_f) continue;
                                            const size_t i = tb + 4 * (g3 + 8 * gq + 4 * half) + rt;
                                            if (f32_ord(acc[rt][ct][g]) >= thr[ct] && i < N) {
                                                const uint32_t pos = atomicAdd(counts + q, 1u);
                                                if (pos < KP) clist[q * KP + pos] = (uint32_t)i;
                                            }
                                        }
                                }
                            }
                        }
                    }
                } else
#ifdef INNR_GEMM_PROBE_SKIPHIT  // tools/gemm_probe.hip: thresholds + fast reject only, never the append path
                if (__any(hit[0] || hit[1]) && dump != nullptr) {
#else
                if (__any(hit[0] || hit[1])) {
#endif
#ifdef INNR_GEMM_PROBE_COUNT  // tools/gemm_probe.hip: how often the append path runs and how much it appends
                    if (lane == 0) atomicAdd(errflag + 8, 1u);
                    atomicAdd(errflag + 9, (uint32_t)hit[0] + (uint32_t)hit[1]);
                    const long long t_hit0 = __builtin_readcyclecounter();
#endif
                    unsigned long long admitted_by[2] = {0ull, 0ull};  // lanes whose query (2*lane + ct) admitted something
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const int ql = 64 * w + 2 * C + ct;
                        uint64_t* lq = my_lists + (size_t)ql * cap;
                        bool admitted = false;
                        {
                            // One compare + branch per value on the way past the 64 sites: "not (v < t)" with t the float
                            // whose order key is thr is a superset of "key(v) >= thr" (it also passes NaNs and -0 vs +0
                            // ties; thr = 0, "no bound", maps to a NaN and passes everything). The exact key test follows
                            // inside. The key conversion per site made this scan ~8K cycles per entry -- and a wave in
                            // here holds up its whole block at the next K-step barrier. (Walking the values with a
                            // runtime loop over a per-wave LDS stage instead -- one copy of the append code, kernel 12.5
                            // instead of 33 KB -- was tried: 18K cycles per entry instead of 7.5K, +1.2 ms.)
                            const float thr_f = ord_f32(thr[ct]);
#pragma unroll
                            for (int gq = 0; gq < 4; ++gq) {
                                const bool ghit = hit[ct] && gbest[ct][gq * NG / 4] >= thr_raw[ct];
                                if (!__any(ghit)) continue;  // wave-uniform: most visits touch one group of one query column
                                if (ghit) {
#pragma unroll
                                    for (int g3 = 0; g3 < 4; ++g3)
#pragma unroll
                                        for (int rt = 0; rt < 4; ++rt) {
                                            const int g = 4 * gq + g3;
                                            if (acc[rt][ct][g] < thr_f) continue;
                                            const uint32_t o = f32_ord(acc[rt][ct][g]);
                                            const size_t i = tb + 4 * (g3 + 8 * gq + 4 * half) + rt;
                                            if (o >= thr[ct] && i < N) {
                                                // the chip-wide bound is re-derived (the expensive half of a visit) for one
                                                // admitted candidate in kEpiPubEvery (the including kernel's: kPubEvery, or the
                                                // screened split filter's own cadence): the bound of a query moves by ~1/KP of
                                                // itself per admission, a few admissions of lag cost next to nothing
                                                admitted = admitted || (((uint32_t)i & (kEpiPubEvery - 1)) == 0);
#ifdef INNR_GEMM_PROBE_COUNT
                                                atomicAdd(errflag + 10, 1u);
#endif
                                                cand_append(lq, &s.cnt[ql], cap, cand_make(o, (uint32_t)i), errflag);
                                                gthr_raise(gslots + (q0 + ql) * (size_t)(kSlotMul * KP), kSlotMul * KP, o, (uint32_t)i);
                                            }
                                        }
                                }
                            }
                        }
                        admitted_by[ct] = __ballot(admitted);
                    }
#ifdef INNR_GEMM_PROBE_COUNT
                    const long long t_hit1 = __builtin_readcyclecounter();
#endif
                    // re-derive the chip-wide bound of every query that admitted something: the whole wave reads the KP
                    // slots of one query at a time (two lanes hold the same query pair: only the lower half reports)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        unsigned long long m = admitted_by[ct];
                        m = (m | (m >> 32)) & 0xffffffffull;  // lanes l and l+32 own the same two queries
                        while (m) {
                            const int L = __builtin_ctzll(m);
                            m &= m - 1;
                            const size_t qg = q0 + 64 * wu + 2 * L + ct;  // wave-uniform
                            if (kSlotMul == 1) gthr_publish_scalar(gslots + qg * (size_t)KP, gthr + qg, KP, lane);
                            else gthr_publish_select<(kSlotMul * (16 * R - 64) + 63) / 64>(gslots + qg * (size_t)(kSlotMul * KP), gthr + qg, KP, lane, kk, kmargin[qg]);  // KP == 16 R - 64 (cand_cap)
                        }
                    }
#ifdef INNR_GEMM_PROBE_COUNT
                    const long long t_hit2 = __builtin_readcyclecounter();
                    if (lane == 0) {
                        atomicAdd(reinterpret_cast<unsigned long long*>(errflag + 14), (unsigned long long)(t_hit1 - t_hit0));
                        atomicAdd(reinterpret_cast<unsigned long long*>(errflag + 16), (unsigned long long)(t_hit2 - t_hit1));
                    }
#endif
                    __builtin_amdgcn_wave_barrier();
                    // compact the lists of this wave's queries that are running out of room
                    const uint32_t c = __hip_atomic_load(&s.cnt[64 * w + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    unsigned long long need = __ballot(c > cap - kGemmBurst);
                    while (need) {
                        const int j = __builtin_ctzll(need);
                        need &= need - 1;
                        const int ql = 64 * w + j;
                        const uint32_t cj = __builtin_amdgcn_readlane(c, j);
                        uint32_t t;
                        const uint32_t keep = wave_compact<R>(my_lists + (size_t)ql * cap, cj, KP, &t);
                        if (lane == 0) {
                            s.cnt[ql] = keep;
                            s.thr[ql] = t;
                            // a list's own KP-th best is a valid chip-wide bound too
                            if (t > __hip_atomic_load(&gthr[q0 + ql], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                                __hip_atomic_fetch_max(&gthr[q0 + ql], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
#ifdef INNR_GEMM_PROBE_COUNT
                    if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(errflag + 12), (unsigned long long)(__builtin_readcyclecounter() - t_hit0));
#endif
                }
            }
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int g = 0; g < 16; ++g) acc[rt][ct][g] = 0.0f;
            if (MODE != 1 && MODE != 3) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) gload1_agent(tg_next[ct], gthr + q0 + 64 * wu + ct, 8u * (uint32_t)(lane & 31));
            }
