// solve_w4_run.inc -- one ADMM run of the four-wave kernel: the loop of solve_wave.hip::
// solve_w4_body between a run's start and its write-back, textually included there.  It reads the
// body's locals by name; w, nsw and pc are the run-time ones, or, in the per-role copies of the
// GL 4 instantiation (admm_run<W>), the ones re-formed from the compile-time wave index
        double* const cw = L.cor + w * 8;                 // c_w rows < 8
        const double* const cwh = L.cor + (h ? 32 : w * 8);  // the half's correction (upper half: zeros)
        while (iter < stop_at) {
            ++iter;
            // rhs = sigma x_prev - q + A' (rho z_prev - y), column pc: the lower half sums
            // the list's first KH entries, the upper half the rest, one permlane32 swap
            {
                double wv[KH];
#pragma unroll
                for (int k = 0; k < KH; ++k) wv[k] = lds_at(ch2.e[k] >> 16);
                double v;
                if constexpr (EL) {
                    // sigma x - q of the lane's column (upper: the eliminated one, whose list it
                    // adds; zero entries on the other lanes), then the upper half's b_p share
                    // carries -ec b_pe
                    double we[LE];
#pragma unroll
                    for (int k = 0; k < LE; ++k) we[k] = lds_at(el.e[k] >> 16);
                    bj = sigma * X - Q;
#pragma unroll
                    for (int k = 0; k < LE; ++k) bj += ea[k] * we[k];
                    v = low ? bj : -(ec * bj);
                } else {
                    v = low ? sigma * X - Q : 0.0;
                }
#pragma unroll
                for (int k = 0; k < KH; ++k) v += ca[k] * wv[k];
                const unsigned vlo = (unsigned)__double2loint(v), vhi = (unsigned)__double2hiint(v);
                const auto l2 = __builtin_amdgcn_permlane32_swap(vlo, vlo, false, false);
                const auto h2 = __builtin_amdgcn_permlane32_swap(vhi, vhi, false, false);
                const double v0 = __hiloint2double((int)h2[0], (int)l2[0]);
                const double v1 = __hiloint2double((int)h2[1], (int)l2[1]);
                if (low) L.rb[pc] = colv ? v0 + v1 : 0.0;
            }
            __syncthreads();
            PH(1)
            if constexpr (DK) {
                // x~[pc] = M^{-1}[pc] b: the half's NB0 + NB1 columns (broadcast reads, one address
                // per half-wave), four FMA chains, one permlane32 swap
                const double* const rbh = L.rb + S * h;
                double a[4] = {0.0, 0.0, 0.0, 0.0};
                // software-pipelined in windows of DKW values: window k + 1's reads are issued
                // before window k's FMAs (two windows in flight; all 27 reads at once spill)
                constexpr int NE = NB0 + NB1, NWIN = (NE + DKW - 1) / DKW;
                double v[2][DKW];
                auto issue = [&](int k, double (&dst)[DKW]) __attribute__((always_inline)) {
#pragma unroll
                    for (int c = 0; c < DKW; c += 2) {
                        const int e = k * DKW + c;  // block h column e, or block 2 + h column e - NB0
                        if (e < NE) ld2(rbh + (e < NB0 ? e : 2 * S + e - NB0), dst[c], dst[c + 1]);
                    }
                };
                issue(0, v[0]);
#pragma unroll
                for (int k = 0; k < NWIN; ++k) {
                    if (k + 1 < NWIN) issue(k + 1, v[(k + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c = 0; c < DKW; ++c)
                        if (k * DKW + c < NE) a[c & 3] += Kr[k * DKW + c] * v[k & 1][c];
                    __builtin_amdgcn_sched_barrier(0);
                }
                const double th = (a[0] + a[1]) + (a[2] + a[3]);
                const unsigned lo = (unsigned)__double2loint(th), hi = (unsigned)__double2hiint(th);
                const auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
                const auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
                const double xn = __hiloint2double((int)h2[0], (int)l2[0]) + __hiloint2double((int)h2[1], (int)l2[1]);
                if (low) L.xt[pc] = xn;
                const double xnew = alpha * xn + (1.0 - alpha) * X;
                DX = xnew - X;
                X = xnew;
            } else {
            // WV: every pair's b_j is read at once (blocks j >= w too: read and not used), so
            // that wave 3 waits for LDS once and not once per branch of the pair nest, and
            // phase B's b_w reads are issued ahead of the reduction (they depend on nothing of
            // phase A): they return while its DPP steps and the c_w round trip run.  c_w still
            // goes through L.cor: taking it from the reduction's lanes by v_readlane was
            // measured slower in three forms (DESIGN.md §16)
            double vb[WV ? 16 : 1];
            if constexpr (WV) {
                double sa = 0.0;
                if (w > 0) {
                    double bj[NB - 1][4];
#pragma unroll
                    for (int j = 0; j < NB - 1; ++j) {
                        ld2(L.rb + j * S + 4 * ch, bj[j][0], bj[j][1]);
                        ld2(L.rb + j * S + 4 * ch + 2, bj[j][2], bj[j][3]);
                    }
                    double acc[NB - 1] = {0.0, 0.0, 0.0};
#pragma unroll
                    for (int j = 0; j < NB - 1; ++j) {
                        if (j < w) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[j] += ga[j][e] * bj[j][e];
                        }
                    }
                    sa = (acc[0] + acc[1]) + acc[2];
                }
#pragma unroll
                for (int c = 0; c < 16; c += 2) ld2(L.rb + w * S + 16 * h + c, vb[c], vb[c + 1]);
                const double cs = reduce8(sa);
                if (w > 0) cw[rr] = cs;
            } else {
            // A: c_w = sum_{j<w} G_wj b_j (rows < 8), wave w only
            if (w > 0) {
                // one accumulator per pair (wave 3: three 4-deep FMA chains instead of one 12-deep)
                double acc[NB - 1] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < NB - 1; ++j) {
                    if (j < w) {
                        double bj[4];
                        ld2(L.rb + j * S + 4 * ch, bj[0], bj[1]);
                        ld2(L.rb + j * S + 4 * ch + 2, bj[2], bj[3]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[j] += ga[j][e] * bj[e];
                    }
                }
                cw[rr] = reduce8((acc[0] + acc[1]) + acc[2]);
            }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            PH(12)
            // B: t_w[r] = S_w^{-1}[r] (b_w + c_w): half-row sums, permlane32 swap
            double t;
            {
                constexpr int QE = (QR + 1) & ~1;  // c_w's nonzero rows (< amax), read in pairs
                double v[16], cc[QE];
                if constexpr (WV) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) v[c] = vb[c];
                } else {
#pragma unroll
                    for (int c = 0; c < 16; c += 2) ld2(L.rb + w * S + 16 * h + c, v[c], v[c + 1]);
                }
#pragma unroll
                for (int c = 0; c < QE; c += 2) ld2(cwh + c, cc[c], cc[c + 1]);
#pragma unroll
                for (int c = 0; c < QR; ++c) v[c] += cc[c];
                double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < 16; ++c) a[c & 3] += SB[c] * v[c];
                const double th = (a[0] + a[1]) + (a[2] + a[3]);
                const unsigned lo = (unsigned)__double2loint(th), hi = (unsigned)__double2hiint(th);
                const auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
                const auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
                const double t0 = __hiloint2double((int)h2[0], (int)l2[0]);  // lower half's
                const double t1 = __hiloint2double((int)h2[1], (int)l2[1]);  // upper half's
                t = t0 + t1;
                if (low && r < 8) L.tv[w * 8 + r] = t;
            }
            __syncthreads();
            PH(13)
            // C: x~_w[r] = t + sum_s G_{pair_s}[q][r] t_{j_s}[q]  (slots split over the halves;
            // rows q < QR: the G blocks are zero from row amax on)
            {
                constexpr int QE = (QR + 1) & ~1;  // t rows read in pairs
                // the wave's slot count (wave 0: 2, waves 1-2: 1, wave 3: 0): slots no half
                // of the wave has a pair for are skipped, not read as the zero pair (LDS
                // return bandwidth is shared with the CU's other workgroup)
                double gv[2][QE], tq[2][QE];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (s < nsw) {
#pragma unroll
                        for (int q = 0; q < QE; ++q) gv[s][q] = q < QR ? gc[s][q] : 0.0;
#pragma unroll
                        for (int q = 0; q < QE; q += 2) lds_at2(tslot[s] + q * 8, tq[s][q], tq[s][q + 1]);
                    } else {
#pragma unroll
                        for (int q = 0; q < QE; ++q) gv[s][q] = tq[s][q] = 0.0;
                    }
                }
                double a0 = 0.0, a1 = 0.0;
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int q = 0; q < QR; q += 2) {
                        if constexpr (ROLES) {
                            // (the second slot's products are rounded before they are added, as
                            // in every other instantiation: there the multiply sits under the
                            // s < nsw test and the add after it, in two basic blocks, which the
                            // compiler does not contract into an fma; with nsw a constant it
                            // would, and wave 0's x~ would move in the last bit)
                            const bool sep = s == 1 && s < nsw;
                            const double p0 = gv[s][q] * tq[s][q];
                            a0 += sep ? rounded(p0) : p0;
                            if (q + 1 < QR) {
                                const double p1 = gv[s][q + 1] * tq[s][q + 1];
                                a1 += sep ? rounded(p1) : p1;
                            }
                        } else {
                        a0 += gv[s][q] * tq[s][q];
                        if (q + 1 < QR) a1 += gv[s][q + 1] * tq[s][q + 1];
                        }
                    }
                const double d = a0 + a1;
                const unsigned lo = (unsigned)__double2loint(d), hi = (unsigned)__double2hiint(d);
                const auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
                const auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
                const double d0 = __hiloint2double((int)h2[0], (int)l2[0]);
                const double d1 = __hiloint2double((int)h2[1], (int)l2[1]);
                const double xn = t + (d0 + d1);
                if (low) L.xt[pc] = xn;
                double xl = xn;  // x~ of the lane's column
                if constexpr (EL) {
                    if (!low) {
                        xl = ed * bj - ec * xn;
                        if (pe >= 0) L.xt[pe] = xl;
                    }
                }
                const double xnew = alpha * xl + (1.0 - alpha) * X;
                DX = xnew - X;
                X = xnew;
            }
            }  // !DK
            __syncthreads();
            PH(14)
            // rows: z~ = A x~ ; relaxed + projected z ; y ; next w (waves wholly past the
            // padded rows skip it: their lanes would only repeat the inert last row)
            if (rows_wave) {
                double xv[K], ar[K];
#pragma unroll
                for (int k = 0; k < K; ++k) xv[k] = lds_at(rg.e[k] >> 16);
                // DK: the row's A values read with x~ (the dense rows leave no registers to
                // keep them across the run)
#pragma unroll
                for (int k = 0; k < K; ++k) ar[k] = DK ? lds_at(rg.e[k] & 0xFFFFu) : av[k];
                const double lo = rlo, up = rup;
                double zt = ar[0] * xv[0];
#pragma unroll
                for (int k = 1; k < K; ++k) zt += ar[k] * xv[k];
                const double zr = alpha * zt + (1.0 - alpha) * Z;
                const double zn = __builtin_fmin(__builtin_fmax(zr + rvi * y, lo), up);
                const double dd = rv * (zr - zn);
                Z = zn;
                dy = dd;
                y += dd;
                L.w[ri] = rv * zn - y;
            }
            __syncthreads();
            PH(3)
        }
