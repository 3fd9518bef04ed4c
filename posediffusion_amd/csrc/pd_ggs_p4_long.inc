// P4 of one GGS iteration of pd_ggs_long_kernel (textually included by it): thread tid < 256 of waves 0 .. 3 = frame tid, where
// pd_ggs_p4.inc has lane = frame on wave 0.  Every expression of a frame is that file's; the sums over the frames (the four dL/dA totals,
// |g|^2, |x . mask|^2, and the focal mean in decode_all_long) are wave_allsum within each of the four frame waves, then
// (w0 + w1) + (w2 + w3) through L.red -- one fixed tree for every N, and with N <= 64 waves 1 .. 3 add +0: the value wave 0 alone forms there.
// ALL eight waves pass through here (the barriers of those sums are workgroup barriers; every branch around them is block-uniform) and all
// of them compute the same coef / done / stepped / last_* values.
// In scope: L (LdsLong), P, S, D, N, b, wg, tid, lane, wave, inv_M, stepped, trace_row, last_print, last_cnt, last_loss.
            // ---- P4 (thread = frame): totals, early exit, quaternion/focal chain, clip, momentum SGD ----
            {
                float xr[9], mom[9];
#pragma unroll
                for (int c = 0; c < 9; ++c) xr[c] = mom[c] = 0.0f;
                if (tid < PD_GGS_LONG_FRAMES) {
                    params_load(L.xst, tid, xr);
                    params_load(L.mst, tid, mom);
                }
                const float s_sum = L.cam[6], s_cnt = L.cam[7], s_cl = L.ctl[2];
                float ga[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (S.update_FL) {                                        // (wave-uniform; only the focal-length chain reads them: 300 of the 700 iterations)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float w = wave_allsum(tid < N ? L.gA[tid * 4 + c] : 0.0f);
                        if (wave < 4 && lane == 0) L.red[c * 4 + wave] = w;
                    }
                    __syncthreads();
#pragma unroll
                    for (int c = 0; c < 4; ++c) ga[c] = (L.red[c * 4 + 0] + L.red[c * 4 + 1]) + (L.red[c * 4 + 2] + L.red[c * 4 + 3]);
                }
                last_print = s_cl * inv_M;
                last_cnt = s_cnt;
                // len(valid) / n_frames < min_matches -> break   (geometry_guided_sampling.py:104-108)
                const bool done = (!P.eval_only) && P.min_matches > 0 && (s_cnt < (float)P.min_matches * (float)N);
                if (!done) {
                    const float inv_cnt = pd_rcp(s_cnt);
                    const float loss = s_sum * inv_cnt;                   // valid.mean()  :110
                    last_loss = loss;
                    float g[9];
#pragma unroll
                    for (int c = 0; c < 9; ++c) g[c] = 0.0f;
                    if (tid < N) {
                        if (S.update_T) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) g[c] = L.gT[tid * 3 + c] * inv_cnt;
                        }
                        if (S.update_R) {
                            // R = I + two_s * Pm(q): chain rule to the (unnormalised) quaternion
                            const float r = xr[3], i = xr[4], j = xr[5], kq = xr[6];
                            const float n2 = r * r + i * i + j * j + kq * kq;
                            const float rn2 = pd_rcp(n2);
                            const float ts = 2.0f * rn2;
                            float gR[9];
#pragma unroll
                            for (int c = 0; c < 9; ++c) gR[c] = L.gR[tid * 9 + c];
                            const float gts = gR[0] * -(j * j + kq * kq) + gR[1] * (i * j - kq * r) + gR[2] * (i * kq + j * r) +
                                              gR[3] * (i * j + kq * r) + gR[4] * -(i * i + kq * kq) + gR[5] * (j * kq - i * r) +
                                              gR[6] * (i * kq - j * r) + gR[7] * (j * kq + i * r) + gR[8] * -(i * i + j * j);
                            float h[9];
#pragma unroll
                            for (int c = 0; c < 9; ++c) h[c] = ts * gR[c];
                            const float qs = gts * (-4.0f * rn2 * rn2);
                            const float gq_r = -kq * h[1] + j * h[2] + kq * h[3] - i * h[5] - j * h[6] + i * h[7] + qs * r;
                            const float gq_i = j * h[1] + kq * h[2] + j * h[3] - 2.0f * i * h[4] - r * h[5] + kq * h[6] +
                                               r * h[7] - 2.0f * i * h[8] + qs * i;
                            const float gq_j = -2.0f * j * h[0] + i * h[1] + r * h[2] + i * h[3] + kq * h[5] - r * h[6] +
                                               kq * h[7] - 2.0f * j * h[8] + qs * j;
                            const float gq_k = -2.0f * kq * h[0] - r * h[1] + i * h[2] + r * h[3] - 2.0f * kq * h[4] +
                                               j * h[5] + i * h[6] + j * h[7] + qs * kq;
                            g[3] = gq_r * inv_cnt;
                            g[4] = gq_i * inv_cnt;
                            g[5] = gq_j * inv_cnt;
                            g[6] = gq_k * inv_cnt;
                        }
                        if (S.update_FL) {
                            // A00 = 1/(f sc), A02 = -cx/(f sc): dA/df ; mean over frames ; exp ; clamp mask
                            const float fbx = L.cam[4], fby = L.cam[5];
                            const float kx = pd_rcp(fbx * fbx * D.sc), ky = pd_rcp(fby * fby * D.sc), rNn = pd_rcp((float)N);
                            const float gfx = (ga[1] * D.cx - ga[0]) * kx;
                            const float gfy = (ga[3] * D.cy - ga[2]) * ky;
                            const float4 fl4 = *(const float4 *)&L.fl[tid * 4];      // (focal x, y | clamp masks x, y)
                            g[7] = gfx * rNn * fl4.x * fl4.z * inv_cnt;
                            g[8] = gfy * rNn * fl4.y * fl4.w * inv_cnt;
                        }
                    }
                    if (P.eval_only) {
                        if (tid < N) {
                            int lo_ = tid;
                            asm volatile("" : "+v"(lo_));     // address arithmetic of this rare branch stays here (not hoisted: registers)
#pragma unroll
                            for (int c = 0; c < 9; ++c) P.grad_out[((size_t)b * P.N + lo_) * 9 + c] = g[c];
                        }
                        if (tid == 0 && wg == 0) {
                            P.loss_out[b * 4 + 0] = loss;
                            P.loss_out[b * 4 + 1] = s_cnt;
                            P.loss_out[b * 4 + 2] = last_print;
                            P.loss_out[b * 4 + 3] = 0.0f;
                        }
                    } else {
                        // masked-norm clip (:114-121) + SGD momentum step (:122)
                        float gn2 = 0.0f, xn2 = 0.0f;
#pragma unroll
                        for (int c = 0; c < 9; ++c) {
                            gn2 += g[c] * g[c];
                            xn2 += (fabsf(g[c]) > 0.0f) ? xr[c] * xr[c] : 0.0f;
                        }
                        {
                            const float gw = wave_allsum(gn2), xw = wave_allsum(xn2);
                            if (wave < 4 && lane == 0) {
                                L.red[16 + wave] = gw;
                                L.red[20 + wave] = xw;
                            }
                        }
                        __syncthreads();
                        const float gnorm = pd_sqrt((L.red[16] + L.red[17]) + (L.red[18] + L.red[19]));
                        const float xnorm = pd_sqrt((L.red[20] + L.red[21]) + (L.red[22] + L.red[23]));
                        const float max_norm = P.alpha * xnorm * pd_rcp(P.lr);
                        const float coef = fminf(max_norm * pd_rcp(gnorm + 1e-6f), 1.0f);
#pragma unroll
                        for (int c = 0; c < 9; ++c) {
                            const float gc = g[c] * coef;
                            mom[c] = (stepped == 0) ? gc : P.momentum * mom[c] + gc;
                            xr[c] = xr[c] - P.lr * mom[c];
                        }
                        ++stepped;
                        if (P.trace && wg == 0 && trace_row < P.trace_iters) {
                            float *tr = P.trace + ((size_t)b * P.trace_iters + trace_row) * (N * 9 + 3);
                            if (tid < N) {
                                int lo_ = tid;
                                asm volatile("" : "+v"(lo_));
#pragma unroll
                                for (int c = 0; c < 9; ++c) tr[lo_ * 9 + c] = xr[c];
                            }
                            if (tid == 0) {
                                tr[N * 9 + 0] = loss;
                                tr[N * 9 + 1] = s_cnt;
                                tr[N * 9 + 2] = gnorm;
                            }
                        }
                        ++trace_row;
                        if (tid < PD_GGS_LONG_FRAMES) {
                            params_store(L.xst, tid, xr);
                            params_store(L.mst, tid, mom);
                        }
                        // only what this stage moves is decoded again (:144-151 detach the rest; the parameters a stage leaves alone keep their bits)
                        decode_all_long(L, xr, tid, N, D, S.update_R != 0, S.update_T != 0, S.update_FL != 0);
                    }
                }
                if (tid == 0) L.ctl[0] = (done || P.eval_only) ? 1.0f : 0.0f;
            }
