// Epilogue of the 256 x 256 f16mx tile (eight waves of 128 x 64; accumulator (i, j)[r] = row 16 i + 4 q4 + r, column 16 j + r16 of
// the wave's block): fused pooling, or the four MX planes / fp32 rows through an LDS staging image. Textually included by the
// tile body of tdnn_mx.hip, which defines: p, stats, rsm, b, t0, n0, out_len, tid, lane, wave, wm, wn, q4, acc, MX_PRM_OFF and -- FLAT (flat row
// tiles, plane output): tile row m is the output row of entry R0 + m of p.row_map -- FLAT, R0.
    const int rows_valid = out_len - t0;
    float ebias[4], esc[4], esh[4];
    {
        const float* prm = reinterpret_cast<const float*>(rsm + MX_PRM_OFF);       // written before the first barrier of the K-loop
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cl = wn * 64 + j * 16 + (lane & 15);
            ebias[j] = prm[cl];
            esc[j] = prm[256 + cl];
            esh[j] = prm[512 + cl];
        }
    }
    if constexpr (OUT == MX_OUT_STATS && FLAT) {
        // fused StatsPooling on flat row tiles (flat_stats_runs, pooled_stats.h): the finished values replace the accumulators, then one partial sum per run
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = mx_act(acc[i][j][r] + ebias[j], ACT) * esc[j] + esh[j];
        flat_stats_runs(acc, R0, rows_valid, wm, lane,
                        [&](int m, int& t_m, int& len_m, int& bb) {
                            const i32x4 e = flat_row(m);
                            t_m = __builtin_amdgcn_readfirstlane(e.y);
                            len_m = __builtin_amdgcn_readfirstlane(e.z);
                            bb = __builtin_amdgcn_readfirstlane(e.w);
                        },
                        [&](int bb, int slot, int j, double s, double q) {
                            const int n = n0 + wn * 64 + j * 16 + (lane & 15);
                            if (n < p.units) stats_out(stats, p, bb, slot, n, s, q);
                        });
        return;
    } else if constexpr (OUT == MX_OUT_STATS) {
        // fused StatsPooling (stats_pooling.py:231-240): per column the sums of the wave's 128 rows (pooled_sums16, pooled_stats.h)
        const int rv = rows_valid - wm * 128;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const PooledSums t = pooled_sums16<8, false>(lane, rv, [&](int i, int r) { return mx_act(acc[i][j][r] + ebias[j], ACT) * esc[j] + esh[j]; });
            const int n = n0 + wn * 64 + j * 16 + (lane & 15);
            if (lane < 16 && n < p.units) stats_out(stats, p, b, pool_block128().slot_of(t0 + wm * 128), n, t.s, t.q);
        }
        return;
    } else {
        __syncthreads();                                 // every fragment read is done: the LDS becomes the store staging area
        // WAVE-PRIVATE staging: a wave's 64 columns are two whole 32-unit chunks, so the rows it encodes and stores are the rows it
        // staged itself -- 64 rows x 64 columns per pass in a region of its own (pitch 68 floats: conflict-free both ways), and no
        // workgroup barrier between the phases of a pass (LDS operations of one wave complete in order). The image shared by all
        // waves -- a wave encoding one chunk for every wave row -- closed each phase with a barrier: 2.3 of the epilogue's 7.5 us.
        float* et = reinterpret_cast<float*>(rsm) + wave * (64 * MX_EPW_PITCH);
        const bool affine = p.scale != nullptr;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {           // rows wm * 128 + pass * 64 .. + 63
            // accumulators -> staging image. The (launch-uniform) `affine` test sits outside the element loops: inside them the
            // compiler kept it as a branch per element, and those 64 branches per pass were half of the epilogue's time.
            auto to_staging = [&](auto aff) {
                constexpr bool AFF = decltype(aff)::value;
#pragma unroll
                for (int ih = 0; ih < 4; ++ih) {
                    const int i = pass * 4 + ih;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int col = j * 16 + (lane & 15);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int srow = ih * 16 + q4 * 4 + r;
                            float v = acc[i][j][r] + ebias[j];
                            if constexpr (OUT == MX_OUT_PLANES) {
                                // the planes saturate at the largest half (mx_encode32 expects clamped values): one v_med3 does the
                                // ReLU and the clamp when no affine follows (the BatchNorm is normally folded into the next layer)
                                if constexpr (AFF) v = __builtin_amdgcn_fmed3f(mx_act(v, ACT) * esc[j] + esh[j], -65504.0f, 65504.0f);
                                else v = __builtin_amdgcn_fmed3f(v, ACT == KTF_ACT_RELU ? 0.0f : -65504.0f, 65504.0f);
                            } else {
                                v = mx_act(v, ACT);
                                if constexpr (AFF) v = v * esc[j] + esh[j];
                            }
                            et[srow * MX_EPW_PITCH + col] = v;
                        }
                    }
                }
            };
            if (affine) to_staging(std::true_type{}); else to_staging(std::false_type{});
            const int m0 = wm * 128 + pass * 64;          // tile row of the wave's staged row 0
            if constexpr (OUT == MX_OUT_PLANES) {
                // (1) lane = staged row: it encodes the row's two chunks; the 64 lanes are 64 consecutive rows of ONE chunk, so the
                //     e2m1 / scale stores write consecutive records; the half piece goes back into the staging image, in place.
                // (2) the wave streams each chunk's half pieces out as 16-byte pieces of consecutive records: 1 KiB of consecutive
                //     bytes per store instruction (store issue is per instruction).
                // first record (chunk 0) of tile row m: (b * nch_out) * Tout + t; a chunk adds chunk * Tout
                auto row_rec = [&](int srow) -> int64_t {
                    if constexpr (FLAT) {
                        const i32x4 e = flat_row(m0 + srow);
                        return (int64_t)(e.x - e.y) * p.nch_out + e.y;
                    } else {
                        return (int64_t)b * p.nch_out * p.Tout + t0 + m0 + srow;
                    }
                };
                const int64_t rec_lane = row_rec(lane);
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const int chunk = (n0 >> 5) + wn * 2 + ch;
                    const int64_t rec = rec_lane + (int64_t)chunk * p.Tout;
                    float* src = et + lane * MX_EPW_PITCH + ch * 32;
                    if (m0 + lane < rows_valid && chunk < p.nch_out) {
                        float v[32];
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const f32x4 t = *reinterpret_cast<const f32x4*>(src + k * 4);
                            v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
                        }
                        u32x4 hp[4], l4, h4;
                        unsigned sw_;
                        mx_encode32(v, hp, l4, h4, sw_);
#pragma unroll
                        for (int k = 0; k < 4; ++k) *reinterpret_cast<u32x4*>(src + k * 4) = hp[k];
                        __builtin_nontemporal_store(l4, reinterpret_cast<u32x4*>(p.yl4 + rec * 16));
                        __builtin_nontemporal_store(h4, reinterpret_cast<u32x4*>(p.y4 + rec * 16));
                        __builtin_nontemporal_store(sw_, reinterpret_cast<unsigned*>(p.ys + rec * 4));
                    }
                }
                int64_t hrec[4];                         // records (chunk 0) of the four rows this lane streams half pieces of
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    // flat row tiles: the record of staged row s is the one lane s looked up above (it fits 32 bits: ktf_tdnn_mx_flat's size
                    // guard) -- a cross-lane read instead of four more table lookups (a division or a global load each) per lane and pass
                    if constexpr (FLAT) hrec[n] = __shfl((int)rec_lane, n * 16 + (lane >> 2), 64);
                    else hrec[n] = row_rec(0) + n * 16 + (lane >> 2);
                }
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const int chunk = (n0 >> 5) + wn * 2 + ch;
                    if (chunk < p.nch_out) {
                        const unsigned char* hsrc = reinterpret_cast<const unsigned char*>(et + ch * 32) + (lane & 3) * 16;
                        char* hdst = p.yh + (int64_t)chunk * p.Tout * 64 + (lane & 3) * 16;
                        if (rows_valid >= 256) {         // whole tile (uniform): all reads in flight, then the stores back to back
                            u32x4 hv[4];
#pragma unroll
                            for (int n = 0; n < 4; ++n)
                                hv[n] = *reinterpret_cast<const u32x4*>(hsrc + (n * 16 + (lane >> 2)) * (MX_EPW_PITCH * 4));
#pragma unroll
                            for (int n = 0; n < 4; ++n)
                                __builtin_nontemporal_store(hv[n], reinterpret_cast<u32x4*>(hdst + hrec[n] * 64));
                        } else {
#pragma unroll
                            for (int n = 0; n < 4; ++n) {
                                const int srow = n * 16 + (lane >> 2);
                                if (m0 + srow < rows_valid) {
                                    const u32x4 v = *reinterpret_cast<const u32x4*>(hsrc + srow * (MX_EPW_PITCH * 4));
                                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(hdst + hrec[n] * 64));
                                }
                            }
                        }
                    }
                }
            } else {
                const int nl = (lane & 15) * 4;
                const int n = n0 + wn * 64 + nl;
#pragma unroll
                for (int sp = 0; sp < 16; ++sp) {
                    const int srow = sp * 4 + (lane >> 4);
                    const int m = m0 + srow;
                    if (m < rows_valid) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(et + srow * MX_EPW_PITCH + nl);
                        float* yp = p.yf + ((int64_t)b * p.Tout + t0 + m) * p.ldy + n;
                        if (n + 4 <= p.units && (p.ldy & 3) == 0) {
                            *reinterpret_cast<f32x4*>(yp) = v;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (n + e < p.units) yp[e] = v[e];
                        }
                    }
                }
            }
        }
    }
