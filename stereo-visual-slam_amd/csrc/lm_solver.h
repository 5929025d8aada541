// lm_solver.h -- the solver around the per-observation maths of lm_device.h, shared by the window LM kernels: lm_window_kernel and
// pose_only_wave_kernel (lm_kernels.hip) and ba_resident_kernel (ba_resident.hip); lm_window_kernel keeps its own damping rule and
// pnp_wave_kernel its whole loop (the notes there say why).  One copy each of
//   * the reduced system's blocked right-looking Cholesky and its backward substitution (reduced_solve), over an accessor for S,
//   * g2o's Levenberg damping rule (LmDamping) and the vslam_lm_stats writes that report it,
//   * the trial pose exp(x) * T,
//   * the adaptive chi2 threshold of the classification.
// Everything is forced inline: a kernel keeps its own shared-memory struct, launch bounds and register budget.
// (The pose graph and full BA solvers -- PCG, another damping loop -- live in pg_solver.h.)
#pragma once
#include "lm_device.h"

namespace vslam {

// ------------------------------------------------------------------------------------------------- where element (r, c) of S lives
// An accessor offers "pointer to the B doubles of row r of block (I, K)" (I >= K: the lower triangle) and nothing else.
template <int BS>
struct DenseRows { // row-major np x np
    static constexpr int B = BS;
    double* S; int np;
    __device__ __forceinline__ double* row(int I, int K, int r) const { return S + (B * I + r) * np + B * K; }
};
template <int BS>
struct PackedBlocks { // block-packed lower triangle: block (I, K) is the (I (I + 1) / 2 + K)-th run of B x B doubles
    static constexpr int B = BS;
    double* S;
    __device__ __forceinline__ double* row(int I, int K, int r) const { return S + (I * (I + 1) / 2 + K) * (B * B) + B * r; }
};

// the instants reduced_solve reports to its clock hook (a callable taking one of these; NoClock for a kernel without phase clocks)
enum { kClkPanel, kClkPanelBarrier, kClkTrailing, kClkTrailingBarrier, kClkFactored, kClkFlagBarrier, kClkBackward };
struct NoClock { __device__ __forceinline__ void operator()(int) const {} };

// Solves S x = bs for the reduced system of nk block rows by NT threads (all of the workgroup; barriers inside).  S and bs are overwritten
// (L below the diagonal blocks, y), Ld (24 doubles per block row) and rdiag take the factored diagonal blocks and their reciprocal
// diagonals, xp the solution -- or zeros when the system is not positive definite (or `ok` came in false): the return value says which.
// *flag is the workgroup's "factorisation failed" word: zero or set by an earlier phase on entry, zero on return.
//
// Cholesky S = L L^T, RIGHT-looking over 6x6 block columns (np = 6 nk), two barriers per block column:
//   P1  every lane that owns a row of the panel below block (J, J) factors the 6x6 diagonal block in registers (redundantly:
//       cheaper than one lane + a broadcast) and solves its row against it, in place; the right-hand side rides along as one
//       more row (L y = b is solved by the factorisation itself: only the backward substitution is left afterwards)
//   P2  the trailing blocks (I, K), J < K <= I, take  -= X_I X_K^T  with one lane per block ROW: 6 outputs from 6 + 36 operands.
// The left-looking form it replaces recomputed every element of a block column as a dot product over all earlier columns with one
// lane per ELEMENT: 2 LDS operands per FMA, and its column update was bound by LDS bandwidth (in-kernel clocks, per block column:
// update 1.84 k cycles, diagonal + rows 2.4 k, barriers 0.55 k).  L_JJ goes to a side array (Ld): nothing reads it before the solve.
template <int NT, class Acc, class Clock>
__device__ __forceinline__ bool reduced_solve(const Acc S, double* bs, double* Ld, double* rdiag, double* xp, int* flag, int nk, int tid, int lane,
                                              int wave, bool ok, Clock&& clk) {
    constexpr int B = Acc::B, TRI = B * (B + 1) / 2, LdStride = (TRI + 3) & ~3; // (a block's triangle in Ld: 24 doubles for B = 6)
    static_assert(B % 2 == 0, "rows are moved as double2");
    static_assert(B == 6 && LdStride == 24, "the callers' Ld holds 24 doubles per block row; the backward substitution carries np = B nk <= 128 unknowns in two values per lane of one wave");
    const int np = B * nk;
    for (int J = 0; J < nk && ok; ++J) {
        const int m = nk - J - 1, nrows = m * B;
        const bool rhs_row = tid == NT - 1;
        if (tid < nrows || tid == 0 || rhs_row) {
            double D[TRI]; // lower triangle, row-major: (i,j) -> i*(i+1)/2 + j
#pragma unroll
            for (int i = 0; i < B; ++i) {
                const double* dj = S.row(J, J, i);
#pragma unroll
                for (int j = 0; j <= i; ++j) D[i * (i + 1) / 2 + j] = dj[j];
            }
            bool good = true;
            double rd[B];
#pragma unroll
            for (int j = 0; j < B; ++j) {
                double d = D[j * (j + 1) / 2 + j];
#pragma unroll
                for (int kk = 0; kk < j; ++kk) d -= D[j * (j + 1) / 2 + kk] * D[j * (j + 1) / 2 + kk];
                if (!(d > 0.0) || !isfinite(d)) good = false;
                rd[j] = rsqrt_nr(d); // the dependent chain of the factorisation: no IEEE sqrt / division on it
                D[j * (j + 1) / 2 + j] = d * rd[j];
#pragma unroll
                for (int i = j + 1; i < B; ++i) {
                    double v = D[i * (i + 1) / 2 + j];
#pragma unroll
                    for (int kk = 0; kk < j; ++kk) v -= D[i * (i + 1) / 2 + kk] * D[j * (j + 1) / 2 + kk];
                    D[i * (i + 1) / 2 + j] = v * rd[j];
                }
            }
            if (tid < nrows || rhs_row) {
                double* rowv = rhs_row ? &bs[B * J] : S.row(J + 1 + tid / B, J, tid % B);
                double x[B];
#pragma unroll
                for (int c = 0; c < B; ++c) {
                    double v = rowv[c];
#pragma unroll
                    for (int kk = 0; kk < c; ++kk) v -= x[kk] * D[c * (c + 1) / 2 + kk];
                    x[c] = v * rd[c];
                }
#pragma unroll
                for (int c = 0; c < B; ++c) rowv[c] = x[c];
            }
            if (tid == 0) {
                if (!good) *flag = 1;
#pragma unroll
                for (int i = 0; i < TRI; ++i) Ld[LdStride * J + i] = D[i];
#pragma unroll
                for (int i = 0; i < B; ++i) rdiag[B * J + i] = rd[i];
            }
        }
        clk(kClkPanel);
        __syncthreads();
        clk(kClkPanelBarrier);
        if (*flag) { ok = false; break; } // uniform
        // P2: trailing update.  Items: (block pair (a, b), a >= b, of the m block rows below; row r) and, for the right-hand side, one
        // item per block b
        const int npair = m * (m + 1) / 2, nitem = npair * B + m;
        for (int t = tid; t < nitem; t += NT) {
            const double* xi; double* out; int Kb;
            if (t < npair * B) {
                const int pr = t / B, r = t - B * pr;
                int a = 0, rem = pr;
                while (rem > a) { rem -= a + 1; ++a; }
                const int Ib = J + 1 + a; Kb = J + 1 + rem;
                xi = S.row(Ib, J, r); out = S.row(Ib, Kb, r);
            } else { Kb = J + 1 + (t - npair * B); xi = &bs[B * J]; out = &bs[B * Kb]; }
            const double2* xi2 = reinterpret_cast<const double2*>(xi);
            double2* o2 = reinterpret_cast<double2*>(out);
            double2 av[B / 2], o[B / 2];
#pragma unroll
            for (int i = 0; i < B / 2; ++i) av[i] = xi2[i];
#pragma unroll
            for (int i = 0; i < B / 2; ++i) o[i] = o2[i];
            double v[B];
#pragma unroll
            for (int i = 0; i < B / 2; ++i) { v[2 * i] = o[i].x; v[2 * i + 1] = o[i].y; }
#pragma unroll
            for (int c = 0; c < B; ++c) {
                const double2* xk = reinterpret_cast<const double2*>(S.row(Kb, J, c));
                double2 bv[B / 2];
#pragma unroll
                for (int i = 0; i < B / 2; ++i) bv[i] = xk[i];
                double s = av[0].x * bv[0].x + av[0].y * bv[0].y;
#pragma unroll
                for (int i = 1; i < B / 2; ++i) s = s + (av[i].x * bv[i].x + av[i].y * bv[i].y);
                v[c] -= s;
            }
#pragma unroll
            for (int i = 0; i < B / 2; ++i) o2[i] = make_double2(v[2 * i], v[2 * i + 1]);
        }
        clk(kClkTrailing);
        __syncthreads();
        clk(kClkTrailingBarrier);
    }
    clk(kClkFactored);
    if (*flag) ok = false;
    __syncthreads();
    clk(kClkFlagBarrier);
    if (tid == 0) *flag = 0;
    if (ok) {
        // backward substitution L^T x = y by wave 0, block by block from the last: lane i carries t_i = y_i - sum over the finished
        // unknowns (and t_{i+64}: np <= 128).  Per block: its six right-hand sides go to every lane (readlane), every lane solves the
        // 6x6 triangle L_JJ^T x = t redundantly (L_JJ from the side array, wave-uniform reads), and the unknowns below take
        // t_i -= sum_c L[6J+c][i] x_c with the six rows of L read along i (consecutive lanes, consecutive addresses).
        if (wave == 0) {
            double u0 = lane < np ? bs[lane] : 0.0, u1 = lane + 64 < np ? bs[lane + 64] : 0.0;
            for (int J = nk - 1; J >= 0; --J) {
                double Lr0[B], Lr1[B], Ldj[TRI], rdj[B], t[B], x[B];
#pragma unroll
                for (int c = 0; c < B; ++c) {
                    Lr0[c] = lane < B * J ? S.row(J, lane / B, c)[lane % B] : 0.0;
                    Lr1[c] = (B * J > 64 && lane + 64 < B * J) ? S.row(J, (lane + 64) / B, c)[(lane + 64) % B] : 0.0;
                    rdj[c] = rdiag[B * J + c];
                }
#pragma unroll
                for (int i = 0; i < TRI; ++i) Ldj[i] = Ld[LdStride * J + i];
#pragma unroll
                for (int c = 0; c < B; ++c) {
                    const int r = B * J + c; // wave-uniform
                    t[c] = r >= 64 ? readlane_f64(u1, r - 64) : readlane_f64(u0, r);
                }
#pragma unroll
                for (int c = B - 1; c >= 0; --c) {
                    double v = t[c];
#pragma unroll
                    for (int k = c + 1; k < B; ++k) v -= Ldj[k * (k + 1) / 2 + c] * x[k];
                    x[c] = v * rdj[c];
                }
                if (lane == 0)
#pragma unroll
                    for (int c = 0; c < B; ++c) xp[B * J + c] = x[c];
#pragma unroll
                for (int c = 0; c < B; ++c) { u0 = fma(-Lr0[c], x[c], u0); u1 = fma(-Lr1[c], x[c], u1); }
            }
        }
        clk(kClkBackward);
    } else {
        for (int i = tid; i < np; i += NT) xp[i] = 0;
    }
    __syncthreads();
    return ok;
}

// ------------------------------------------------------------------------------------------------- g2o's Levenberg damping
// lambda0 = 1e-5 max |diag H|; a trial with gain rho = (chi - chi_trial) / scale > 0 is accepted: lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)),
// ni = 2; a rejected one: lambda *= ni, ni *= 2.  At most 10 trials per iteration; the loop ends with an iteration of 10 trials or zero gain.
struct LmDamping {
    double lambda = 0, ni = 2, rho_gain = 0;
    int qmax = 0; // trials of this iteration
    __device__ __forceinline__ void init(double max_diag) { lambda = 1e-5 * max_diag; ni = 2; }
    __device__ __forceinline__ void begin_iteration() { rho_gain = 0; qmax = 0; }
    // one trial: its cost (ok = false: the solve failed, the trial counts as DBL_MAX) against the current one; returns "accepted"
    __device__ __forceinline__ bool step(double currentChi, double tempChi, double scale, bool ok) {
        if (!ok) tempChi = 1.7976931348623157e308;
        rho_gain = (currentChi - tempChi) / scale;
        const bool accept = rho_gain > 0 && isfinite(tempChi);
        if (accept) {
            double alpha = 1. - pow(2 * rho_gain - 1, 3);
            alpha = fmin(alpha, 2. / 3.);
            lambda *= fmax(1. / 3., alpha);
            ni = 2;
        } else {
            lambda *= ni;
            ni *= 2;
        }
        ++qmax;
        return accept;
    }
    __device__ __forceinline__ bool again() const { return (rho_gain < 0) && qmax < 10; }
    __device__ __forceinline__ bool iteration_ends() const { return qmax == 10 || rho_gain == 0; }
};

// the statistics of iteration `it` / of the whole loop, by the kernel's one writing lane (st may be null)
__device__ __forceinline__ void lm_stats_iter(vslam_lm_stats* st, int it, double currentChi, const LmDamping& lm) {
    if (st && it < VSLAM_LM_MAX_ITERS) { st->chi2_iter[it] = currentChi; st->lambda_iter[it] = lm.lambda; st->trials_iter[it] = lm.qmax; }
}
__device__ __forceinline__ void lm_stats_final(vslam_lm_stats* st, int it, int total_trials, double currentChi, const LmDamping& lm) {
    if (st) { st->iterations = it; st->total_trials = total_trials; st->chi2_final = currentChi; st->lambda_final = lm.lambda; }
}

// ------------------------------------------------------------------------------------------------- trial pose T' = exp(x) * T, expanded
__device__ __forceinline__ void trial_pose(const double* x, const double* T, double* T_trial, double* Rt_trial) {
    double E[7];
    se3::exp(x, E);
    se3::mul(E, T, T_trial);
    expand_pose(T_trial, Rt_trial);
}

// ------------------------------------------------------------------------------------------------- adaptive chi2 threshold
// optimization.cpp:224-252: start at th (the Huber delta) and double it up to five times while at most half of the edges are inliers.
// counts(th, ti, in, out) gives the tallies at threshold th = delta 2^ti.  Returns the number of doublings.
template <class Counts>
__device__ __forceinline__ int chi2_threshold(double& th, Counts&& counts) {
    int ti = 0;
    for (int iteration = 0; iteration < 5; ++iteration) {
        double in, out;
        counts(th, ti, in, out);
        const double ratio = in / (in + out);
        if (ratio > 0.5) break; // uniform
        th *= 2; ++ti;
    }
    return ti;
}

} // namespace vslam
