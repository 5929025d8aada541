// fullba_kernels.hip -- full bundle adjustment (include/vslam_hip.h "full bundle adjustment").
//
// One persistent workgroup per problem runs every Levenberg-Marquardt iteration of its problem, the design of posegraph_kernels.hip (the set-up
// phases and the edge cost pass the two solvers share are in pg_solver.h): linearise the observations and edges, eliminate the landmarks, solve the reduced camera system S = U + edges - W V^-1 W' by preconditioned conjugate gradients
// that never form it, back-substitute, try the step, accept or reject.  No grid-wide synchronisation, no host round trip.
//
// An observation's Jacobians factor through A = de/dP (3 x 3, P the point in the camera): Jp = A [I, -P^], Jl = A R.  With B = rho' A'A (symmetric,
// entry 01 is zero) and g = rho' A'e every block of the normal equations is a function of (P, B, g) and the keyframe's rotation:
//   U_o = [I; P^] B [I, -P^],  V_o = R' B R,  W_o = [I; P^] B R,  Jp' rho' e = [g; P x g],  Jl' rho' e = R' g,
// so a stored observation is 11 doubles (FBA_STORE) -- or nothing: the other form recomputes (P, B) from the accepted state in every phase.
//
// Passes.  Per linearisation: observations (lane per observation: cost, P, B, g), landmarks (lane per landmark over its contiguous observations:
// V_l, b_l), keyframes (lane per keyframe over its incidence list: U_k + edge blocks, b_k).  Per LM iteration: landmarks (V'^-1, V'^-1 b_l),
// keyframes (the preconditioner block and the reduced right-hand side).  Per PCG iteration: landmarks u_l = V'^-1 sum W_o' p_k; incidence positions
// (lane per position: c_q = W_o u_l) and edges; keyframes y_k = (U_k + lambda D_k) p_k - sum c_q + edge terms, the sum walking the keyframe's
// positions upwards, i.e. in ascending observation order; vector updates.
//
// Determinism: pg_device.h's sums (index k in lane k % 64, xor butterfly per aligned block of 64, block sums ascending), list walks in ascending
// order, integer atomics only.  None of it depends on the workgroup width or on the other problems of the batch.
#include <algorithm>

#include "pg_solver.h"
#include "se3_device.h"
#include "vslam_internal.h"

namespace vslam {

// 256 lanes, one wave per SIMD: the keyframe passes hold a 6 x 6 block, its update and the edge Jacobians at once (318 VGPRs + AGPRs).  The same source
// built for 512 lanes (256 registers per lane) spills 64 - 81 VGPRs to a private segment, which tests/test_kernel_resources.py does not allow.
constexpr int kFbaThreads = 256;
constexpr int kFbaLin = 11;   // doubles per stored observation: P (3), B (00 02 11 12 22), g (3)

struct FbaState {
    int32_t* status;                              // n_problems (first slot: vslam_full_ba_status_dev reads it)
    double *lin, *cq;                             // per observation: the stored linearisation; c_q per incidence position (6)
    uint8_t* oact;                                // per observation: active in this call
    int32_t *kinc, *ktmp;                         // per observation: the keyframes' incidence lists (sorted / as filled)
    double *V, *bl, *Vi, *tl, *ul, *Xn;           // per landmark: V_l (6), b_l (3), V'^-1 (6), V'^-1 b_l (3), u_l (3), candidate point (3)
    int32_t *lstart, *lend, *lseen;               // per landmark: its observation range and whether one of them is active
    double *H, *F, *Rk;                           // per keyframe: U_k + edge blocks (36), preconditioner block (36), rotation at the linearisation (9)
    double *b, *br, *x, *r, *z, *p, *y, *D;       // per keyframe, 6 each
    double* Tnew;                                 // per keyframe, 7
    int32_t *held, *kstart, *estart, *kcur, *ecur; // per keyframe: held flag, offsets of the two incidence lists (N + 1 each), fill cursors
    double *PQ, *res, *te;                        // per edge: Pi Qi Pj Qj (36), residual (6), W J_other p_other per side (12)
    int32_t *einc, *etmp;                         // per edge x 2: 2 e + side
    double *pk0, *pk1, *pk2, *po, *pe, *pl;       // block sums: three per 64 keyframes, one per 64 observations / edges / landmarks
};

struct FbaArgs {
    vslam_full_ba b;
    vslam_full_ba_params p;
    double* T_out;
    double* X_out;
    vslam_full_ba_stats* stats;
    FbaState s;
};

namespace {

struct FbaCam { double fx, fy, cx, cy, bf, huber; };

PG_DEV bool fba_stereo(float d) { return d >= 0.0f; }   // (false for NaN)
PG_DEV void fba_point(const double* R, const double* t, const double* X, double* P) {
#pragma unroll
    for (int i = 0; i < 3; ++i) P[i] = R[i * 3] * X[0] + R[i * 3 + 1] * X[1] + R[i * 3 + 2] * X[2] + t[i];
}
PG_DEV double fba_residual(const FbaCam& c, const double* P, float u, float v, float d, bool stereo, double* e) {
    const double iz = 1.0 / P[2];
    e[0] = (double)u - (c.fx * P[0] * iz + c.cx);
    e[1] = (double)v - (c.fy * P[1] * iz + c.cy);
    e[2] = stereo ? (double)d - c.bf * iz : 0.0;
    return e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
}
PG_DEV void fba_huber(double s, double delta, double& rho, double& w) {
    const double d2 = delta * delta;
    if (!(delta > 0) || s <= d2) { rho = s; w = 1.0; }
    else { const double r = sqrt(s); rho = 2 * r * delta - d2; w = delta / r; }
}
// B = w A'A (00 02 11 12 22) and g = w A'e
PG_DEV void fba_lin(const FbaCam& c, const double* P, const double* e, bool stereo, double w, double* B, double* g) {
    const double iz = 1.0 / P[2], iz2 = iz * iz;
    const double a00 = -c.fx * iz, a02 = c.fx * P[0] * iz2, a11 = -c.fy * iz, a12 = c.fy * P[1] * iz2, a22 = stereo ? c.bf * iz2 : 0.0;
    B[0] = w * a00 * a00; B[1] = w * a00 * a02; B[2] = w * a11 * a11; B[3] = w * a11 * a12; B[4] = w * (a02 * a02 + a12 * a12 + a22 * a22);
    g[0] = w * a00 * e[0]; g[1] = w * a11 * e[1]; g[2] = w * (a02 * e[0] + a12 * e[1] + a22 * e[2]);
}
PG_DEV void fba_Bmul(const double* B, const double* q, double* s) {
    s[0] = B[0] * q[0] + B[1] * q[2];
    s[1] = B[2] * q[1] + B[3] * q[2];
    s[2] = B[1] * q[0] + B[3] * q[1] + B[4] * q[2];
}
PG_DEV void fba_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
PG_DEV void fba_Rv(const double* R, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = R[i * 3] * v[0] + R[i * 3 + 1] * v[1] + R[i * 3 + 2] * v[2];
}
PG_DEV void fba_Rtv(const double* R, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = R[i] * v[0] + R[3 + i] * v[1] + R[6 + i] * v[2];
}
// symmetric 3 x 3 (00 01 02 11 12 22) times a vector
PG_DEV void fba_Smul(const double* S, const double* v, double* o) {
    o[0] = S[0] * v[0] + S[1] * v[1] + S[2] * v[2];
    o[1] = S[1] * v[0] + S[3] * v[1] + S[4] * v[2];
    o[2] = S[2] * v[0] + S[4] * v[1] + S[5] * v[2];
}
// Hk (6 x 6 row-major) += sign [I; P^] C [I, -P^] for a symmetric C (00 01 02 11 12 22)
PG_DEV void fba_add_block(double* Hk, const double* C, const double* P, double sign) {
    const double Cf[9] = {C[0], C[1], C[2], C[1], C[3], C[4], C[2], C[4], C[5]};
    double G[9], Q[9];   // G = C P^, Q = P^ G
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        G[i * 3] = Cf[i * 3 + 1] * P[2] - Cf[i * 3 + 2] * P[1];
        G[i * 3 + 1] = Cf[i * 3 + 2] * P[0] - Cf[i * 3] * P[2];
        G[i * 3 + 2] = Cf[i * 3] * P[1] - Cf[i * 3 + 1] * P[0];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Q[j] = P[1] * G[6 + j] - P[2] * G[3 + j];
        Q[3 + j] = P[2] * G[j] - P[0] * G[6 + j];
        Q[6 + j] = P[0] * G[3 + j] - P[1] * G[j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Hk[i * 6 + j] += sign * Cf[i * 3 + j];
            Hk[i * 6 + 3 + j] -= sign * G[i * 3 + j];
            Hk[(3 + i) * 6 + j] -= sign * G[j * 3 + i];
            Hk[(3 + i) * 6 + 3 + j] -= sign * Q[i * 3 + j];
        }
}
// inverse of a symmetric 3 x 3 (00 01 02 11 12 22) that must be positive definite (Sylvester); false leaves zeros
PG_DEV bool fba_inv3(const double* S, double* Si) {
    const double a = S[0], b = S[1], c = S[2], d = S[3], e = S[4], f = S[5];
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double det = a * c00 + b * c01 + c * c02;
    const bool ok = a > 0 && a * d - b * b > 0 && det > 0 && pg_finite(det);
    const double id = ok ? 1.0 / det : 0.0;
    Si[0] = c00 * id; Si[1] = c01 * id; Si[2] = c02 * id; Si[3] = (a * f - c * c) * id; Si[4] = (b * c - a * e) * id; Si[5] = (a * d - b * b) * id;
    return ok;
}

} // namespace

template <int T, bool STORE>
__global__ __launch_bounds__(T) void full_ba_kernel(FbaArgs a) {
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const FbaState& s = a.s;
    __shared__ int sh_scan[T];
    __shared__ int sh_cnt[8];   // free keyframes, singular flag, observations dropped, active observations

    // ---- the problem's ranges
    const int G = a.b.n_problems;
    const int n0 = a.b.d_kf_off[g], n1 = a.b.d_kf_off[g + 1], m0 = a.b.d_lm_off[g], m1 = a.b.d_lm_off[g + 1];
    const int o0 = a.b.d_obs_off[g], o1 = a.b.d_obs_off[g + 1], e0 = a.b.d_edge_off[g], e1 = a.b.d_edge_off[g + 1];
    const int ok = __syncthreads_and(pg_own_range<T>(a.b.d_kf_off, G, g, a.b.total_kfs, tid) & pg_own_range<T>(a.b.d_lm_off, G, g, a.b.total_lms, tid) &
                                     pg_own_range<T>(a.b.d_obs_off, G, g, a.b.total_obs, tid) & pg_own_range<T>(a.b.d_edge_off, G, g, a.b.total_edges, tid));
    vslam_full_ba_stats st;
    st.chi2_init = st.chi2_final = 0; st.lambda = a.p.lambda_init; st.lm_iters = st.pcg_iters = st.n_free = st.n_obs_dropped = 0; st.status = 0; st.reserved = 0;
    if (!ok) {
        st.status = VSLAM_FBA_BAD_INDEX;
        pg_write_stats(st, s.status, a.stats, g, tid);
        return;
    }
    const int N = n1 - n0, M = m1 - m0, O = o1 - o0, E = e1 - e0;
    const FbaCam cam = {a.b.K4[0], a.b.K4[1], a.b.K4[2], a.b.K4[3], a.b.bf, a.b.huber_delta};
    const int32_t* okf = a.b.d_obs_kf + o0; const int32_t* olm = a.b.d_obs_lm + o0;
    const float* ouv = a.b.d_obs_uv + (size_t)o0 * 2; const float* odisp = a.b.d_obs_disp ? a.b.d_obs_disp + o0 : nullptr;
    const uint8_t* oin = a.b.d_obs_active ? a.b.d_obs_active + o0 : nullptr;
    const PgEdges ed = {E, a.b.d_edge_i + e0, a.b.d_edge_j + e0, a.b.d_edge_Z + (size_t)e0 * 7, a.b.d_edge_w + (size_t)e0 * 6,
                        a.b.d_edge_active ? a.b.d_edge_active + e0 : nullptr, s.PQ + (size_t)e0 * 36, s.res + (size_t)e0 * 6};
    const double* Tin = a.b.d_T + (size_t)n0 * 7; const double* Xin = a.b.d_xyz + (size_t)m0 * 3;
    double* To = a.T_out + (size_t)n0 * 7; double* Xo = a.X_out + (size_t)m0 * 3;
    double* lin = s.lin + (size_t)o0 * kFbaLin; double* cq = s.cq + (size_t)o0 * 6;
    uint8_t* oact = s.oact + o0; int32_t* kinc = s.kinc + o0; int32_t* ktmp = s.ktmp + o0;
    double* Vl = s.V + (size_t)m0 * 6; double* bl = s.bl + (size_t)m0 * 3; double* Vi = s.Vi + (size_t)m0 * 6; double* tl = s.tl + (size_t)m0 * 3;
    double* ul = s.ul + (size_t)m0 * 3; double* Xn = s.Xn + (size_t)m0 * 3;
    int32_t* lstart = s.lstart + m0; int32_t* lend = s.lend + m0; int32_t* lseen = s.lseen + m0;
    double* Hd = s.H + (size_t)n0 * 36; double* Fd = s.F + (size_t)n0 * 36; double* Rk = s.Rk + (size_t)n0 * 9;
    double* vb = s.b + (size_t)n0 * 6; double* vbr = s.br + (size_t)n0 * 6; double* vx = s.x + (size_t)n0 * 6; double* vr = s.r + (size_t)n0 * 6;
    double* vz = s.z + (size_t)n0 * 6; double* vp = s.p + (size_t)n0 * 6; double* vy = s.y + (size_t)n0 * 6; double* vD = s.D + (size_t)n0 * 6;
    double* Tn = s.Tnew + (size_t)n0 * 7;
    int32_t* held = s.held + n0; int32_t* kstart = s.kstart + n0 + g; int32_t* estart = s.estart + n0 + g; int32_t* kcur = s.kcur + n0; int32_t* ecur = s.ecur + n0;
    double* te = s.te + (size_t)e0 * 12;
    int32_t* einc = s.einc + (size_t)e0 * 2; int32_t* etmp = s.etmp + (size_t)e0 * 2;
    double* pk0 = s.pk0 + (n0 >> 6) + g; double* pk1 = s.pk1 + (n0 >> 6) + g; double* pk2 = s.pk2 + (n0 >> 6) + g;
    double* po = s.po + (o0 >> 6) + g; double* pe = s.pe + (e0 >> 6) + g; double* pl = s.pl + (m0 >> 6) + g;
    const int Nr = (N + 63) & ~63, Mr = (M + 63) & ~63, Or = (O + 63) & ~63;

    // ---- the caller's ids and values; poses and points are copied through
    int bad = 0, nonfinite = 0;
    for (int o = tid; o < O; o += T) {
        const int k = okf[o], l = olm[o];
        if (k < 0 || k >= N || l < 0 || l >= M || (o > 0 && olm[o - 1] > l)) bad = 1;
        if (!pg_finite(ouv[(size_t)o * 2]) || !pg_finite(ouv[(size_t)o * 2 + 1])) nonfinite = 1;
        if (odisp && odisp[o] > 3.4028234e38f) nonfinite = 1;   // (+inf; a NaN or a negative value marks a mono observation)
    }
    pg_check_edges<T>(ed, N, tid, bad, nonfinite);
    pg_copy_poses<T>(Tin, To, N, tid, nonfinite);
    for (int l = tid; l < M; l += T) {
        for (int q = 0; q < 3; ++q) {
            const double v = Xin[(size_t)l * 3 + q];
            if (!pg_finite(v)) nonfinite = 1;
            Xo[(size_t)l * 3 + q] = v;
        }
    }
    bad = __syncthreads_or(bad);
    nonfinite = __syncthreads_or(nonfinite);
    if (bad || nonfinite) {
        st.status = (bad ? VSLAM_FBA_BAD_INDEX : 0) | (nonfinite ? VSLAM_FBA_NONFINITE : 0);
        pg_write_stats(st, s.status, a.stats, g, tid);
        return;
    }

    // ---- the observations of the call, the landmarks' ranges, held keyframes and the two incidence lists
    if (tid < 8) sh_cnt[tid] = 0;
    for (int k = tid; k < N; k += T) { held[k] = a.b.d_fixed ? (a.b.d_fixed[n0 + k] != 0) : (k == 0); kcur[k] = 0; ecur[k] = 0; }
    for (int l = tid; l < M; l += T) { lstart[l] = 0; lend[l] = 0; }
    __syncthreads();
    {
        int dropped = 0, nact = 0;
        for (int o = tid; o < O; o += T) {
            const int k = okf[o], l = olm[o];
            if (o == 0 || olm[o - 1] != l) lstart[l] = o;
            if (o == O - 1 || olm[o + 1] != l) lend[l] = o + 1;
            int on = !(oin && !oin[o]);
            if (on) {
                double R[9], X[3], P[3];
                se3::rotmat(To + (size_t)k * 7, R);
#pragma unroll
                for (int q = 0; q < 3; ++q) X[q] = Xo[(size_t)l * 3 + q];
                fba_point(R, To + (size_t)k * 7 + 4, X, P);
                if (!(P[2] > 0)) { on = 0; ++dropped; }
            }
            oact[o] = (uint8_t)on;
            if (on) { atomicAdd(&kcur[k], 1); ++nact; }
        }
        if (dropped) atomicAdd(&sh_cnt[2], dropped);
        if (nact) atomicAdd(&sh_cnt[3], nact);
        for (int e = tid; e < E; e += T) {
            if (!ed.on(e)) continue;
            atomicAdd(&ecur[ed.i[e]], 1); atomicAdd(&ecur[ed.j[e]], 1);
        }
    }
    __syncthreads();
    pg_hold_isolated<T>(held, N, tid, &sh_cnt[0], [&](int k) { return kcur[k] == 0 && ecur[k] == 0; });
    __syncthreads();
    pg_counts_to_offsets<T>(kcur, kstart, N, sh_scan, tid);
    pg_counts_to_offsets<T>(ecur, estart, N, sh_scan, tid);
    for (int o = tid; o < O; o += T) if (oact[o]) ktmp[atomicAdd(&kcur[okf[o]], 1)] = o;
    for (int e = tid; e < E; e += T) {
        if (!ed.on(e)) continue;
        etmp[atomicAdd(&ecur[ed.i[e]], 1)] = 2 * e;
        etmp[atomicAdd(&ecur[ed.j[e]], 1)] = 2 * e + 1;
    }
    __syncthreads();
    pg_sort_lists_by_wave<T>(kstart, ktmp, kinc, N, tid);
    pg_sort_lists_by_wave<T>(estart, etmp, einc, N, tid);
    for (int k = tid; k < N; k += T) {
        for (int q = 0; q < 6; ++q) {
            const size_t o = (size_t)k * 6 + q;
            vb[o] = vbr[o] = vx[o] = vr[o] = vz[o] = vp[o] = vy[o] = vD[o] = 0.0;
        }
    }
    __syncthreads();
    const int n_free = sh_cnt[0], n_dropped = sh_cnt[2], n_act = sh_cnt[3];
    const int Q = kstart[N];   // (= n_act)
    st.n_free = n_free; st.n_obs_dropped = n_dropped;

    // (P, B) of observation o at the accepted state: stored by the last linearisation, or recomputed from it
    auto obs_PB = [&](int o, int k, const double* R, double* P, double* B) {
        if (STORE) {
            const double* lo = lin + (size_t)o * kFbaLin;
#pragma unroll
            for (int q = 0; q < 3; ++q) P[q] = lo[q];
#pragma unroll
            for (int q = 0; q < 5; ++q) B[q] = lo[3 + q];
        } else {
            double X[3], e[3], gq[3], rho, w;
            const int l = olm[o];
#pragma unroll
            for (int q = 0; q < 3; ++q) X[q] = Xo[(size_t)l * 3 + q];
            fba_point(R, To + (size_t)k * 7 + 4, X, P);
            const float d = odisp ? odisp[o] : -1.0f;
            const bool stereo = fba_stereo(d);
            fba_huber(fba_residual(cam, P, ouv[(size_t)o * 2], ouv[(size_t)o * 2 + 1], d, stereo, e), cam.huber, rho, w);
            fba_lin(cam, P, e, stereo, w, B, gq);
        }
    };

    // the cost of the active observations and edges at (Tp, Xp); with `lin` the linearisation is kept for the solver
    auto cost_of = [&](const double* Tp, const double* Xp, bool keep) -> double {
        for (int o = tid; o < Or; o += T) {
            double c = 0;
            if (o < O && oact[o]) {
                const int k = okf[o], l = olm[o];
                double R[9], X[3], P[3], e[3], rho, w;
                se3::rotmat(Tp + (size_t)k * 7, R);
#pragma unroll
                for (int q = 0; q < 3; ++q) X[q] = Xp[(size_t)l * 3 + q];
                fba_point(R, Tp + (size_t)k * 7 + 4, X, P);
                const float d = odisp ? odisp[o] : -1.0f;
                const bool stereo = fba_stereo(d);
                fba_huber(fba_residual(cam, P, ouv[(size_t)o * 2], ouv[(size_t)o * 2 + 1], d, stereo, e), cam.huber, rho, w);
                c = P[2] > 0 ? rho : __builtin_huge_val();
                if (keep) {
                    double B[5], gq[3];
                    fba_lin(cam, P, e, stereo, w, B, gq);
                    double* lo = lin + (size_t)o * kFbaLin;
#pragma unroll
                    for (int q = 0; q < 3; ++q) { lo[q] = P[q]; lo[8 + q] = gq[q]; }
#pragma unroll
                    for (int q = 0; q < 5; ++q) lo[3 + q] = B[q];
                }
            }
            c = pg_wave_sum(c);
            if (lane == 0) po[o >> 6] = c;
        }
        pg_edge_cost_pass<T>(ed, Tp, keep, pe, tid);
        if (keep) {
            for (int k = tid; k < N; k += T) {
                double R[9];
                se3::rotmat(Tp + (size_t)k * 7, R);
#pragma unroll
                for (int q = 0; q < 9; ++q) Rk[(size_t)k * 9 + q] = R[q];
            }
        }
        __syncthreads();
        const double total = pg_sum_parts(po, O) + pg_sum_parts(pe, E);
        __syncthreads();   // (the block sums are free again)
        return total;
    };

    // u_l = V'^-1 sum_o W_o' v_kf(o) over the landmark's active observations, ascending
    auto landmark_phase = [&](const double* v) {
        for (int l = tid; l < M; l += T) {
            double acc[3] = {0, 0, 0}, Vm[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) Vm[q] = Vi[(size_t)l * 6 + q];
            if (lseen[l]) {
                for (int o = lstart[l]; o < lend[l]; ++o) {
                    if (!oact[o]) continue;
                    const int k = okf[o];
                    if (held[k]) continue;   // (v is zero there)
                    double R[9], P[3], B[5], vk[6], qv[3], sv[3], c3[3];
#pragma unroll
                    for (int q = 0; q < 9; ++q) R[q] = Rk[(size_t)k * 9 + q];
#pragma unroll
                    for (int q = 0; q < 6; ++q) vk[q] = v[(size_t)k * 6 + q];
                    obs_PB(o, k, R, P, B);
                    fba_cross(vk + 3, P, c3);
#pragma unroll
                    for (int q = 0; q < 3; ++q) qv[q] = vk[q] + c3[q];
                    fba_Bmul(B, qv, sv);
                    fba_Rtv(R, sv, c3);
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc[q] += c3[q];
                }
            }
            double u[3];
            fba_Smul(Vm, acc, u);
#pragma unroll
            for (int q = 0; q < 3; ++q) ul[(size_t)l * 3 + q] = u[q];
        }
    };

    double cost = cost_of(To, Xo, true);
    st.chi2_init = st.chi2_final = cost;
    double lambda = a.p.lambda_init;
    bool fresh = true;   // the linearisation belongs to (To, Xo) and the blocks have not been built from it yet
    int status = n_dropped ? VSLAM_FBA_DROPPED : 0;
    const int max_iters = (n_free > 0 || n_act > 0) ? a.p.max_iters : 0;

    for (int it = 0; it < max_iters; ++it) {
        if (fresh) {
            // ---- landmarks: V_l = sum R' B R, b_l = -sum R' g
            for (int l = tid; l < M; l += T) {
                double V[6] = {0, 0, 0, 0, 0, 0}, b3[3] = {0, 0, 0};
                int seen = 0;
                for (int o = lstart[l]; o < lend[l]; ++o) {
                    if (!oact[o]) continue;
                    seen = 1;
                    const int k = okf[o];
                    const double* lo = lin + (size_t)o * kFbaLin;
                    double R[9], B[5], gq[3], BR[9], t3[3];
#pragma unroll
                    for (int q = 0; q < 9; ++q) R[q] = Rk[(size_t)k * 9 + q];
#pragma unroll
                    for (int q = 0; q < 5; ++q) B[q] = lo[3 + q];
#pragma unroll
                    for (int q = 0; q < 3; ++q) gq[q] = lo[8 + q];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {   // column c of B R
                        const double rc[3] = {R[c], R[3 + c], R[6 + c]};
                        fba_Bmul(B, rc, t3);
                        BR[c] = t3[0]; BR[3 + c] = t3[1]; BR[6 + c] = t3[2];
                    }
                    // V += R' (B R): entries 00 01 02 11 12 22
                    V[0] += R[0] * BR[0] + R[3] * BR[3] + R[6] * BR[6];
                    V[1] += R[0] * BR[1] + R[3] * BR[4] + R[6] * BR[7];
                    V[2] += R[0] * BR[2] + R[3] * BR[5] + R[6] * BR[8];
                    V[3] += R[1] * BR[1] + R[4] * BR[4] + R[7] * BR[7];
                    V[4] += R[1] * BR[2] + R[4] * BR[5] + R[7] * BR[8];
                    V[5] += R[2] * BR[2] + R[5] * BR[5] + R[8] * BR[8];
                    fba_Rtv(R, gq, t3);
#pragma unroll
                    for (int q = 0; q < 3; ++q) b3[q] -= t3[q];
                }
                lseen[l] = seen;
#pragma unroll
                for (int q = 0; q < 6; ++q) Vl[(size_t)l * 6 + q] = V[q];
#pragma unroll
                for (int q = 0; q < 3; ++q) bl[(size_t)l * 3 + q] = b3[q];
            }
            // ---- keyframes: H_kk = sum U_o + the edges' diagonal blocks, b_k = -sum [g; P x g] - sum J' W r
            for (int k = tid; k < N; k += T) {
                double Hk[36], bk[6];
#pragma unroll
                for (int q = 0; q < 36; ++q) Hk[q] = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) bk[q] = 0;
                if (held[k]) {
                    Hk[0] = Hk[7] = Hk[14] = Hk[21] = Hk[28] = Hk[35] = 1.0;
                } else {
                    for (int q = kstart[k]; q < kstart[k + 1]; ++q) {
                        const double* lo = lin + (size_t)kinc[q] * kFbaLin;
                        double P[3], gq[3], c3[3];
#pragma unroll
                        for (int m = 0; m < 3; ++m) { P[m] = lo[m]; gq[m] = lo[8 + m]; }
                        const double C[6] = {lo[3], 0.0, lo[4], lo[5], lo[6], lo[7]};
                        fba_add_block(Hk, C, P, 1.0);
                        fba_cross(P, gq, c3);
#pragma unroll
                        for (int m = 0; m < 3; ++m) { bk[m] -= gq[m]; bk[3 + m] -= c3[m]; }
                    }
                    for (int q = estart[k]; q < estart[k + 1]; ++q) {
                        const int e = einc[q] >> 1, side = einc[q] & 1;
                        const double* pq = ed.PQ + (size_t)e * 36;
                        double Pa[9], Qa[9], w[6], wr[6], o6[6];
#pragma unroll
                        for (int m = 0; m < 9; ++m) { Pa[m] = pq[side * 18 + m]; Qa[m] = pq[side * 18 + 9 + m]; }
#pragma unroll
                        for (int m = 0; m < 6; ++m) { w[m] = ed.w[(size_t)e * 6 + m]; wr[m] = w[m] * ed.res[(size_t)e * 6 + m]; }
                        pg_JT(Pa, Qa, wr, o6);
#pragma unroll
                        for (int m = 0; m < 6; ++m) bk[m] -= o6[m];
                        pg_JtWJ(Pa, Qa, Pa, Qa, w, Hk);
                    }
                }
#pragma unroll
                for (int q = 0; q < 36; ++q) Hd[(size_t)k * 36 + q] = Hk[q];
#pragma unroll
                for (int q = 0; q < 6; ++q) { vb[(size_t)k * 6 + q] = bk[q]; vD[(size_t)k * 6 + q] = held[k] ? 0.0 : Hk[q * 7]; }
            }
            fresh = false;
            __syncthreads();
        }

        // ---- the damped landmark blocks: V'^-1 and V'^-1 b_l; a block that is not positive definite holds its landmark for this iteration
        {
            int sing = 0;
            for (int l = tid; l < M; l += T) {
                double V[6], Vm[6], b3[3], t3[3];
#pragma unroll
                for (int q = 0; q < 6; ++q) V[q] = Vl[(size_t)l * 6 + q];
                V[0] += lambda * V[0]; V[3] += lambda * V[3]; V[5] += lambda * V[5];
                const bool pd = fba_inv3(V, Vm);
                if (!pd && lseen[l]) sing = 1;
#pragma unroll
                for (int q = 0; q < 3; ++q) b3[q] = bl[(size_t)l * 3 + q];
                fba_Smul(Vm, b3, t3);
#pragma unroll
                for (int q = 0; q < 6; ++q) Vi[(size_t)l * 6 + q] = Vm[q];
#pragma unroll
                for (int q = 0; q < 3; ++q) tl[(size_t)l * 3 + q] = t3[q];
            }
            if (sing) atomicOr(&sh_cnt[1], 1);
        }
        __syncthreads();
        // ---- the preconditioner blocks (H_kk + lambda D_k - sum W_o V'^-1 W_o')^-1 and the reduced right-hand side b_k - sum W_o V'^-1 b_l
        {
            int sing = 0;
            for (int k = tid; k < N; k += T) {
                if (held[k]) continue;
                double Mk[36], bk[6], R[9];
#pragma unroll
                for (int q = 0; q < 36; ++q) Mk[q] = Hd[(size_t)k * 36 + q];
#pragma unroll
                for (int q = 0; q < 6; ++q) { Mk[q * 7] += lambda * vD[(size_t)k * 6 + q]; bk[q] = vb[(size_t)k * 6 + q]; }
#pragma unroll
                for (int q = 0; q < 9; ++q) R[q] = Rk[(size_t)k * 9 + q];
                for (int q = kstart[k]; q < kstart[k + 1]; ++q) {
                    const int o = kinc[q], l = olm[o];
                    double P[3], B[5], Vm[6], BR[9], t3[3], s3[3], c3[3], Tm[9], C[6];
                    obs_PB(o, k, R, P, B);
#pragma unroll
                    for (int m = 0; m < 6; ++m) Vm[m] = Vi[(size_t)l * 6 + m];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double rc[3] = {R[c], R[3 + c], R[6 + c]};
                        fba_Bmul(B, rc, t3);
                        BR[c] = t3[0]; BR[3 + c] = t3[1]; BR[6 + c] = t3[2];
                    }
                    // Tm = (B R) V'^-1 (row i), C = Tm (B R)'
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        fba_Smul(Vm, BR + i * 3, t3);
                        Tm[i * 3] = t3[0]; Tm[i * 3 + 1] = t3[1]; Tm[i * 3 + 2] = t3[2];
                    }
                    C[0] = Tm[0] * BR[0] + Tm[1] * BR[1] + Tm[2] * BR[2];
                    C[1] = Tm[0] * BR[3] + Tm[1] * BR[4] + Tm[2] * BR[5];
                    C[2] = Tm[0] * BR[6] + Tm[1] * BR[7] + Tm[2] * BR[8];
                    C[3] = Tm[3] * BR[3] + Tm[4] * BR[4] + Tm[5] * BR[5];
                    C[4] = Tm[3] * BR[6] + Tm[4] * BR[7] + Tm[5] * BR[8];
                    C[5] = Tm[6] * BR[6] + Tm[7] * BR[7] + Tm[8] * BR[8];
                    fba_add_block(Mk, C, P, -1.0);
                    // s = (B R) V'^-1 b_l
#pragma unroll
                    for (int m = 0; m < 3; ++m) t3[m] = tl[(size_t)l * 3 + m];
#pragma unroll
                    for (int i = 0; i < 3; ++i) s3[i] = BR[i * 3] * t3[0] + BR[i * 3 + 1] * t3[1] + BR[i * 3 + 2] * t3[2];
                    fba_cross(P, s3, c3);
#pragma unroll
                    for (int m = 0; m < 3; ++m) { bk[m] -= s3[m]; bk[3 + m] -= c3[m]; }
                }
                sing |= pg_inv6(Mk);
#pragma unroll
                for (int q = 0; q < 36; ++q) Fd[(size_t)k * 36 + q] = Mk[q];
#pragma unroll
                for (int q = 0; q < 6; ++q) vbr[(size_t)k * 6 + q] = bk[q];
            }
            if (sing) atomicOr(&sh_cnt[1], 1);
        }
        __syncthreads();

        // z = F r and the block sums of r.z (pk1) and r.r (pk2)
        auto precondition = [&]() {
            for (int k = tid; k < Nr; k += T) {
                double rz = 0, rr = 0;
                if (k < N && !held[k]) {
                    double rk[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) rk[q] = vr[(size_t)k * 6 + q];
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        double zq = 0;
#pragma unroll
                        for (int c = 0; c < 6; ++c) zq += Fd[(size_t)k * 36 + q * 6 + c] * rk[c];
                        vz[(size_t)k * 6 + q] = zq;
                        rz += rk[q] * zq; rr += rk[q] * rk[q];
                    }
                }
                rz = pg_wave_sum(rz); rr = pg_wave_sum(rr);
                if (lane == 0) { pk1[k >> 6] = rz; pk2[k >> 6] = rr; }
            }
            __syncthreads();
        };

        // ---- conjugate gradients on S x = b_red, x0 = 0
        for (int k = tid; k < N; k += T) {
#pragma unroll
            for (int q = 0; q < 6; ++q) { vx[(size_t)k * 6 + q] = 0.0; vr[(size_t)k * 6 + q] = held[k] ? 0.0 : vbr[(size_t)k * 6 + q]; }
        }
        precondition();
        double rz = pg_sum_parts(pk1, N), rr = pg_sum_parts(pk2, N);
        const double rr0 = rr;
        for (int k = tid; k < N; k += T) {
#pragma unroll
            for (int q = 0; q < 6; ++q) vp[(size_t)k * 6 + q] = held[k] ? 0.0 : vz[(size_t)k * 6 + q];
        }
        __syncthreads();
        int cg = 0;
        const double tol2 = a.p.pcg_tol * a.p.pcg_tol;
        while (rr0 > 0 && rr > tol2 * rr0) {
            if (cg >= a.p.pcg_max_iters) { status |= VSLAM_FBA_PCG_CAP; break; }
            landmark_phase(vp);
            __syncthreads();
            // incidence positions: c_q = W_o u_l = [s; P x s], s = B R_k u_l
            for (int q = tid; q < Q; q += T) {
                const int o = kinc[q], k = okf[o], l = olm[o];
                double R[9], P[3], B[5], u[3], t3[3], s3[3], c3[3];
#pragma unroll
                for (int m = 0; m < 9; ++m) R[m] = Rk[(size_t)k * 9 + m];
                obs_PB(o, k, R, P, B);
#pragma unroll
                for (int m = 0; m < 3; ++m) u[m] = ul[(size_t)l * 3 + m];
                fba_Rv(R, u, t3);
                fba_Bmul(B, t3, s3);
                fba_cross(P, s3, c3);
#pragma unroll
                for (int m = 0; m < 3; ++m) { cq[(size_t)q * 6 + m] = s3[m]; cq[(size_t)q * 6 + 3 + m] = c3[m]; }
            }
            // edges: per side the other side's W J p
            for (int e = tid; e < E; e += T) {
                if (!ed.on(e)) continue;
                const int i = ed.i[e], j = ed.j[e];
                const double* pq = ed.PQ + (size_t)e * 36;
                double Pm[9], Qm[9], v[6], t1[6], t2[6];
#pragma unroll
                for (int m = 0; m < 9; ++m) { Pm[m] = pq[m]; Qm[m] = pq[9 + m]; }
#pragma unroll
                for (int m = 0; m < 6; ++m) v[m] = vp[(size_t)i * 6 + m];
                pg_J(Pm, Qm, v, t1);
#pragma unroll
                for (int m = 0; m < 9; ++m) { Pm[m] = pq[18 + m]; Qm[m] = pq[27 + m]; }
#pragma unroll
                for (int m = 0; m < 6; ++m) v[m] = vp[(size_t)j * 6 + m];
                pg_J(Pm, Qm, v, t2);
#pragma unroll
                for (int m = 0; m < 6; ++m) { const double w = ed.w[(size_t)e * 6 + m]; te[(size_t)e * 12 + m] = w * t2[m]; te[(size_t)e * 12 + 6 + m] = w * t1[m]; }
            }
            __syncthreads();
            // keyframes: y_k = (H_kk + lambda D_k) p_k - sum c_q + sum J_side' te, and the block sums of p.y
            for (int k = tid; k < Nr; k += T) {
                double py = 0;
                if (k < N && !held[k]) {
                    double yk[6], pk[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) pk[q] = vp[(size_t)k * 6 + q];
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        double acc = lambda * vD[(size_t)k * 6 + q] * pk[q];
#pragma unroll
                        for (int c = 0; c < 6; ++c) acc += Hd[(size_t)k * 36 + q * 6 + c] * pk[c];
                        yk[q] = acc;
                    }
                    for (int q = kstart[k]; q < kstart[k + 1]; ++q) {
#pragma unroll
                        for (int m = 0; m < 6; ++m) yk[m] -= cq[(size_t)q * 6 + m];
                    }
                    for (int q = estart[k]; q < estart[k + 1]; ++q) {
                        const int e = einc[q] >> 1, side = einc[q] & 1;
                        const double* pq = ed.PQ + (size_t)e * 36 + side * 18;
                        double Pm[9], Qm[9], t[6], o6[6];
#pragma unroll
                        for (int m = 0; m < 9; ++m) { Pm[m] = pq[m]; Qm[m] = pq[9 + m]; }
#pragma unroll
                        for (int m = 0; m < 6; ++m) t[m] = te[(size_t)e * 12 + side * 6 + m];
                        pg_JT(Pm, Qm, t, o6);
#pragma unroll
                        for (int m = 0; m < 6; ++m) yk[m] += o6[m];
                    }
#pragma unroll
                    for (int q = 0; q < 6; ++q) { vy[(size_t)k * 6 + q] = yk[q]; py += pk[q] * yk[q]; }
                }
                py = pg_wave_sum(py);
                if (lane == 0) pk0[k >> 6] = py;
            }
            __syncthreads();
            const double py = pg_sum_parts(pk0, N);
            if (!(py > 0) || !pg_finite(py)) break;
            const double alpha = rz / py;
            for (int k = tid; k < N; k += T) {
                if (held[k]) continue;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    vx[(size_t)k * 6 + q] += alpha * vp[(size_t)k * 6 + q];
                    vr[(size_t)k * 6 + q] -= alpha * vy[(size_t)k * 6 + q];
                }
            }
            precondition();
            const double rz_new = pg_sum_parts(pk1, N);
            rr = pg_sum_parts(pk2, N);
            const double beta = rz_new / rz;
            rz = rz_new;
            for (int k = tid; k < N; k += T) {
                if (held[k]) continue;
#pragma unroll
                for (int q = 0; q < 6; ++q) vp[(size_t)k * 6 + q] = vz[(size_t)k * 6 + q] + beta * vp[(size_t)k * 6 + q];
            }
            ++cg;
            __syncthreads();
        }
        st.pcg_iters += cg;
        __syncthreads();   // (a lane that left the loop early has read its block sums)

        // ---- back-substitution dX_l = V'^-1 b_l - u_l(x), the candidate (exp(x) T, X + dX) and |delta|
        landmark_phase(vx);
        for (int k = tid; k < Nr; k += T) {
            double dd = 0;
            if (k < N) {
                double Tk[7], Tc[7];
#pragma unroll
                for (int q = 0; q < 7; ++q) Tk[q] = To[(size_t)k * 7 + q];
                if (held[k]) {
#pragma unroll
                    for (int q = 0; q < 7; ++q) Tc[q] = Tk[q];
                } else {
                    double xk[6], Ex[7];
#pragma unroll
                    for (int q = 0; q < 6; ++q) { xk[q] = vx[(size_t)k * 6 + q]; dd += xk[q] * xk[q]; }
                    se3::exp(xk, Ex);
                    se3::mul(Ex, Tk, Tc);
                }
#pragma unroll
                for (int q = 0; q < 7; ++q) Tn[(size_t)k * 7 + q] = Tc[q];
            }
            dd = pg_wave_sum(dd);
            if (lane == 0) pk0[k >> 6] = dd;
        }
        for (int l = tid; l < Mr; l += T) {   // (the lane that wrote u_l in landmark_phase reads it)
            double dd = 0;
            if (l < M) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double dx = tl[(size_t)l * 3 + q] - ul[(size_t)l * 3 + q];
                    Xn[(size_t)l * 3 + q] = Xo[(size_t)l * 3 + q] + dx;
                    dd += dx * dx;
                }
            }
            dd = pg_wave_sum(dd);
            if (lane == 0) pl[l >> 6] = dd;
        }
        __syncthreads();
        const double step = sqrt(pg_sum_parts(pk0, N) + pg_sum_parts(pl, M));
        const double cost_new = cost_of(Tn, Xn, false);
        st.lm_iters = it + 1;
        if (cost_new < cost) {   // (false for a NaN and for the infinity of a point behind its camera)
            for (int k = tid; k < N; k += T) {
#pragma unroll
                for (int q = 0; q < 7; ++q) To[(size_t)k * 7 + q] = Tn[(size_t)k * 7 + q];
            }
            for (int l = tid; l < M; l += T) {
#pragma unroll
                for (int q = 0; q < 3; ++q) Xo[(size_t)l * 3 + q] = Xn[(size_t)l * 3 + q];
            }
            __syncthreads();
            cost = cost_of(To, Xo, true);   // (the same sum as cost_new, and the linearisation of the next iteration)
            fresh = true;
            lambda = fmax(lambda / 10.0, 1e-12);
        } else {
            lambda *= 10.0;
        }
        if (!(step >= a.p.step_tol)) break;
        if (lambda > 1e12) { status |= VSLAM_FBA_LAMBDA; break; }
    }

    // ---- e'e of every observation at the output state
    if (a.b.d_obs_chi2) {
        for (int o = tid; o < O; o += T) {
            const int k = okf[o], l = olm[o];
            double R[9], X[3], P[3], e[3];
            se3::rotmat(To + (size_t)k * 7, R);
#pragma unroll
            for (int q = 0; q < 3; ++q) X[q] = Xo[(size_t)l * 3 + q];
            fba_point(R, To + (size_t)k * 7 + 4, X, P);
            const float d = odisp ? odisp[o] : -1.0f;
            a.b.d_obs_chi2[o0 + o] = fba_residual(cam, P, ouv[(size_t)o * 2], ouv[(size_t)o * 2 + 1], d, fba_stereo(d), e);
        }
    }
    if (tid == 0) {
        st.chi2_final = cost; st.lambda = lambda;
        st.status = status | (sh_cnt[1] ? VSLAM_FBA_SINGULAR : 0);
        s.status[g] = st.status;
        if (a.stats) a.stats[g] = st;
    }
}

int launch_full_ba(const vslam_full_ba& b, const vslam_full_ba_params& p, int store, double* d_T_out, double* d_xyz_out, vslam_full_ba_stats* d_stats,
                   DevBuf& buf, hipStream_t stream) {
    FbaArgs a;
    a.b = b; a.p = p; a.T_out = d_T_out; a.X_out = d_xyz_out; a.stats = d_stats;
    const size_t G = (size_t)b.n_problems, N = (size_t)b.total_kfs, M = (size_t)b.total_lms, O = (size_t)b.total_obs, E = (size_t)b.total_edges;
    FbaState& s = a.s;
    if (int rc = carve(buf, stream, [&](Layout& l) {
            s.status = l.take<int32_t>(G);
            s.lin = l.take<double>(O * kFbaLin); s.cq = l.take<double>(O * 6);
            s.oact = l.take<uint8_t>(O); s.kinc = l.take<int32_t>(O); s.ktmp = l.take<int32_t>(O);
            s.V = l.take<double>(M * 6); s.bl = l.take<double>(M * 3); s.Vi = l.take<double>(M * 6); s.tl = l.take<double>(M * 3);
            s.ul = l.take<double>(M * 3); s.Xn = l.take<double>(M * 3);
            s.lstart = l.take<int32_t>(M); s.lend = l.take<int32_t>(M); s.lseen = l.take<int32_t>(M);
            s.H = l.take<double>(N * 36); s.F = l.take<double>(N * 36); s.Rk = l.take<double>(N * 9);
            s.b = l.take<double>(N * 6); s.br = l.take<double>(N * 6); s.x = l.take<double>(N * 6); s.r = l.take<double>(N * 6);
            s.z = l.take<double>(N * 6); s.p = l.take<double>(N * 6); s.y = l.take<double>(N * 6); s.D = l.take<double>(N * 6);
            s.Tnew = l.take<double>(N * 7);
            s.held = l.take<int32_t>(N); s.kstart = l.take<int32_t>(N + G); s.estart = l.take<int32_t>(N + G); s.kcur = l.take<int32_t>(N); s.ecur = l.take<int32_t>(N);
            s.PQ = l.take<double>(E * 36); s.res = l.take<double>(E * 6); s.te = l.take<double>(E * 12);
            s.einc = l.take<int32_t>(E * 2); s.etmp = l.take<int32_t>(E * 2);
            s.pk0 = l.take<double>(N / 64 + G + 1); s.pk1 = l.take<double>(N / 64 + G + 1); s.pk2 = l.take<double>(N / 64 + G + 1);
            s.po = l.take<double>(O / 64 + G + 1); s.pe = l.take<double>(E / 64 + G + 1); s.pl = l.take<double>(M / 64 + G + 1);
        })) return rc;
    if (b.n_problems == 0) return VSLAM_OK;
    ProfScope prof__(stream, "full_ba_kernel");
    const dim3 grid(b.n_problems);
    if (store) hipLaunchKernelGGL((full_ba_kernel<kFbaThreads, true>), grid, dim3(kFbaThreads), 0, stream, a);
    else hipLaunchKernelGGL((full_ba_kernel<kFbaThreads, false>), grid, dim3(kFbaThreads), 0, stream, a);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
