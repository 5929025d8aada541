// pg_device.h -- device helpers shared by the persistent-workgroup solvers (posegraph_kernels.hip, fullba_kernels.hip): the deterministic sums
// (an xor butterfly per aligned block of 64 indices, block sums added in ascending order), the pose-pose edge residual and its Jacobian factors
// (include/vslam_hip.h "pose-graph optimisation"), and the 6 x 6 inverses.  What one lane computes is here; the phases a whole workgroup runs with
// them (checks, scans, edge cost, PCG and LM drivers) are in pg_solver.h.
#pragma once
#include "se3_device.h"
#include "vslam_internal.h"

namespace vslam {
namespace {

#define PG_DEV __device__ __forceinline__

PG_DEV bool pg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; } // (false for NaN and +-inf)

PG_DEV double pg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the ascending sum of the block sums every lane forms after the barrier that follows their writes
PG_DEV double pg_sum_parts(const double* part, int count) {
    double s = 0;
    for (int i = 0; i < (count + 63) / 64; ++i) s += part[i];
    return s;
}
PG_DEV double pg_readlane(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

PG_DEV void pg_hat(const double* v, double* M) {
    M[0] = 0; M[1] = -v[2]; M[2] = v[1];
    M[3] = v[2]; M[4] = 0; M[5] = -v[0];
    M[6] = -v[1]; M[7] = v[0]; M[8] = 0;
}
PG_DEV void pg_mm3(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// r = log(Z^-1 Ti Tj^-1); E and Z^-1 for the Jacobians
PG_DEV void pg_residual(const double* Ti, const double* Tj, const double* Z, double* r, double* E, double* Zi) {
    double Tji[7], Tij[7];
    se3::inverse(Z, Zi);
    se3::inverse(Tj, Tji);
    se3::mul(Ti, Tji, Tij);
    se3::mul(Zi, Tij, E);
    se3::log(E, r);
}
PG_DEV double pg_chi2(const double* r, const double* w) {
    double c = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) c += r[i] * w[i] * r[i];
    return c;
}
// P = sign a R, Q = sign (a t^ R + b R) of sign A Ad(T)
PG_DEV void pg_jac(const double* a, const double* bq, const double* T, double sign, double* P, double* Q) {
    double R[9], th[9], tR[9], Q1[9], Q2[9];
    se3::rotmat(T, R);
    pg_hat(T + 4, th);
    pg_mm3(th, R, tR);
    pg_mm3(a, R, P);
    pg_mm3(a, tR, Q1);
    pg_mm3(bq, R, Q2);
#pragma unroll
    for (int i = 0; i < 9; ++i) { P[i] *= sign; Q[i] = sign * (Q1[i] + Q2[i]); }
}
// out = J v for J = [[P, Q], [0, P]]
PG_DEV void pg_J(const double* P, const double* Q, const double* v, double* out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i] = P[i * 3] * v[0] + P[i * 3 + 1] * v[1] + P[i * 3 + 2] * v[2] + Q[i * 3] * v[3] + Q[i * 3 + 1] * v[4] + Q[i * 3 + 2] * v[5];
        out[3 + i] = P[i * 3] * v[3] + P[i * 3 + 1] * v[4] + P[i * 3 + 2] * v[5];
    }
}
// out = J' t
PG_DEV void pg_JT(const double* P, const double* Q, const double* t, double* out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i] = P[i] * t[0] + P[3 + i] * t[1] + P[6 + i] * t[2];
        out[3 + i] = Q[i] * t[0] + Q[3 + i] * t[1] + Q[6 + i] * t[2] + P[i] * t[3] + P[3 + i] * t[4] + P[6 + i] * t[5];
    }
}
// column c of J
PG_DEV void pg_Jcol(const double* P, const double* Q, int c, double* v) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] = c < 3 ? P[i * 3 + c] : Q[i * 3 + (c - 3)];
        v[3 + i] = c < 3 ? 0.0 : P[i * 3 + (c - 3)];
    }
}
// Hacc += Ja' diag(w) Jb (6 x 6 row-major)
PG_DEV void pg_JtWJ(const double* Pa, const double* Qa, const double* Pb, const double* Qb, const double* w, double* Hacc) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double v[6], o[6];
        pg_Jcol(Pb, Qb, c, v);
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] *= w[i];
        pg_JT(Pa, Qa, v, o);
#pragma unroll
        for (int i = 0; i < 6; ++i) Hacc[i * 6 + c] += o[i];
    }
}
// in-place Gauss-Jordan inverse of a symmetric positive definite 6 x 6; a pivot that is not positive is replaced by 1 and reported
PG_DEV bool pg_inv6(double* a) {
    bool bad = false;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double piv = a[p * 6 + p];
        if (!(piv > 0) || !pg_finite(piv)) { bad = true; piv = 1.0; }
        const double inv = 1.0 / piv;
        a[p * 6 + p] = 1.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) a[p * 6 + j] *= inv;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i == p) continue;
            const double f = a[i * 6 + p];
            a[i * 6 + p] = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) a[i * 6 + j] -= f * a[p * 6 + j];
        }
    }
    return bad;
}
// the same with one matrix row per lane (lanes 0..5 of a wave; `row` is this lane's row, a[] its six entries)
PG_DEV bool pg_inv6_rows(double* a, int row) {
    bool bad = false;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double np[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) np[j] = pg_readlane(a[j], p);
        double piv = np[p];
        if (!(piv > 0) || !pg_finite(piv)) { bad = true; piv = 1.0; }
        const double inv = 1.0 / piv;
        np[p] = 1.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) np[j] *= inv;
        const double f = a[p];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double elim = (j == p ? 0.0 : a[j]) - f * np[j];
            a[j] = row == p ? np[j] : elim;
        }
    }
    return bad;
}

} // namespace
} // namespace vslam
