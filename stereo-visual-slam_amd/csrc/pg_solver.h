// pg_solver.h -- the workgroup-level phases shared by the persistent-workgroup solvers (posegraph_kernels.hip, fullba_kernels.hip, DESIGN.md 5.10 and
// 5.11): the checks on the caller's offsets, edges and poses, held nodes, counts to offsets and the two incidence-list sorts, the edge cost and
// linearisation pass, and the stats write.  The leaf arithmetic and the deterministic sums are in pg_device.h.  The Levenberg-Marquardt loop itself
// (build, preconditioner, conjugate gradients, candidate, accept) stays written out in each kernel: DESIGN.md 5.10 says why.
//
// Every function is called by all T lanes of the workgroup with the same arguments; a lane takes the indices tid, tid + T, ... of a loop (so index k
// sits in lane k % 64 and the sums are pg_device.h's).  Each comment says whether the function ends on a barrier.
#pragma once
#include "pg_device.h"

namespace vslam {
namespace {

// one problem's pose-pose edges: node ids relative to the problem's first node, measurement (7), weights (6), optional active flags, and what the
// linearisation keeps per edge: Pi Qi Pj Qj (36) and the residual (6)
struct PgEdges {
    int E;
    const int32_t *i, *j;
    const double *Z, *w;
    const uint8_t* act;
    double *PQ, *res;
    PG_DEV bool on(int e) const { return !(act && !act[e]); }
};

// this lane's share of the check on offset array `off` (G + 1 entries): problem g's range is inside [0, total], in order, and no other problem's offset
// cuts into it (so that a bad neighbour cannot alias this one).  The caller combines the lanes with __syncthreads_and.
template <int T>
PG_DEV int pg_own_range(const int32_t* off, int G, int g, int total, int tid) {
    const int x0 = off[g], x1 = off[g + 1];
    int ok = x0 >= 0 && x1 >= x0 && x1 <= total;
    for (int k = tid; k <= G; k += T) {
        const int v = off[k];
        if (k <= g ? v > x0 : v < x1) ok = 0;
    }
    return ok;
}

// the caller's edges: `bad` for an id outside [0, N) or a self edge, `nonfinite` for a non-finite measurement or a weight that is not finite and >= 0
template <int T>
PG_DEV void pg_check_edges(const PgEdges& ed, int N, int tid, int& bad, int& nonfinite) {
    for (int e = tid; e < ed.E; e += T) {
        const int i = ed.i[e], j = ed.j[e];
        if (i < 0 || i >= N || j < 0 || j >= N || i == j) bad = 1;
        for (int q = 0; q < 7; ++q) if (!pg_finite(ed.Z[(size_t)e * 7 + q])) nonfinite = 1;
        for (int q = 0; q < 6; ++q) { const double w = ed.w[(size_t)e * 6 + q]; if (!pg_finite(w) || w < 0) nonfinite = 1; }
    }
}
// the caller's poses, copied through to the output (the same lane owns node k in every node loop of the kernels)
template <int T>
PG_DEV void pg_copy_poses(const double* Tin, double* To, int N, int tid, int& nonfinite) {
    for (int k = tid; k < N; k += T) {
        for (int q = 0; q < 7; ++q) {
            const double v = Tin[(size_t)k * 7 + q];
            if (!pg_finite(v)) nonfinite = 1;
            To[(size_t)k * 7 + q] = v;
        }
    }
}

// a node without a term is held; the free nodes are counted into *n_free (shared memory, zeroed before).  No barrier.
template <int T, class Isolated>
PG_DEV void pg_hold_isolated(int32_t* held, int N, int tid, int* n_free, Isolated&& isolated) {
    int nfree = 0;
    for (int k = tid; k < N; k += T) {
        if (isolated(k)) held[k] = 1;
        nfree += !held[k];
    }
    if (nfree) atomicAdd(n_free, nfree);
}

// counts -> offsets over the nodes (start[N] is their sum); the counts become fill cursors that restart at the offsets.  Ends on a barrier.
template <int T>
PG_DEV void pg_counts_to_offsets(int32_t* cnt, int32_t* start, int N, int* sh_scan, int tid) {
    const int chunk = (N + T - 1) / T, k0 = min(N, tid * chunk), k1 = min(N, k0 + chunk);
    int sum = 0;
    for (int k = k0; k < k1; ++k) sum += cnt[k];
    sh_scan[tid] = sum;
    __syncthreads();
    int base = 0;
    for (int t = 0; t < tid; ++t) base += sh_scan[t];
    for (int k = k0; k < k1; ++k) { const int d = cnt[k]; start[k] = base; cnt[k] = base; base += d; }
    if (tid == T - 1) start[N] = base;
    __syncthreads();
}

// The atomic fill leaves an incidence list in any order; both sorts leave every list ascending (its entries are distinct).  No barrier.
// A lane per list, insertion in place: thousands of lists of two or three entries (the pose graph's edges).
template <int T>
PG_DEV void pg_sort_lists_by_lane(const int32_t* start, int32_t* inc, int N, int tid) {
    for (int k = tid; k < N; k += T) {
        const int b0 = start[k], b1 = start[k + 1];
        for (int q = b0 + 1; q < b1; ++q) {
            const int v = inc[q];
            int m = q - 1;
            while (m >= b0 && inc[m] > v) { inc[m + 1] = inc[m]; --m; }
            inc[m + 1] = v;
        }
    }
}
// A wave per list, a lane per entry, placed by rank from tmp into out: lists of hundreds (full BA's observations per keyframe).
template <int T>
PG_DEV void pg_sort_lists_by_wave(const int32_t* start, const int32_t* tmp, int32_t* out, int N, int tid) {
    for (int k = tid >> 6; k < N; k += T >> 6) {
        const int b0 = start[k], n = start[k + 1] - b0;
        for (int i = (tid & 63); i < n; i += 64) {
            const int v = tmp[b0 + i];
            int r = 0;
            for (int j = 0; j < n; ++j) r += tmp[b0 + j] < v;
            out[b0 + r] = v;
        }
    }
}

// chi2 of one edge at poses Ti, Tj; with `keep` its Jacobian factors go to pq (36) and its residual to res (6)
PG_DEV double pg_edge_cost(const double* Tip, const double* Tjp, const double* Zp, const double* wp, bool keep, double* pq, double* res) {
    double Ti[7], Tj[7], Z[7], w[6], r[6], Ee[7], Zi[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) { Ti[q] = Tip[q]; Tj[q] = Tjp[q]; Z[q] = Zp[q]; }
#pragma unroll
    for (int q = 0; q < 6; ++q) w[q] = wp[q];
    pg_residual(Ti, Tj, Z, r, Ee, Zi);
    if (keep) {
        double Om[9], U[9], Om2[9], OU[9], UO[9], am[9], bm[9], P[9], Q[9];
        pg_hat(r + 3, Om); pg_hat(r, U);
        pg_mm3(Om, Om, Om2); pg_mm3(Om, U, OU); pg_mm3(U, Om, UO);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            am[q] = -0.5 * Om[q] + Om2[q] * (1.0 / 12.0);
            bm[q] = -0.5 * U[q] + (OU[q] + UO[q]) * (1.0 / 12.0);
        }
        am[0] += 1.0; am[4] += 1.0; am[8] += 1.0;
        pg_jac(am, bm, Zi, 1.0, P, Q);
#pragma unroll
        for (int q = 0; q < 9; ++q) { pq[q] = P[q]; pq[9 + q] = Q[q]; }
        pg_jac(am, bm, Ee, -1.0, P, Q);
#pragma unroll
        for (int q = 0; q < 9; ++q) { pq[18 + q] = P[q]; pq[27 + q] = Q[q]; }
#pragma unroll
        for (int q = 0; q < 6; ++q) res[q] = r[q];
    }
    return pg_chi2(r, w);
}
// the block sums (one per 64 edges) of the active edges' chi2 at poses Tp; with `keep` their linearisation is stored.  No barrier.
template <int T>
PG_DEV void pg_edge_cost_pass(const PgEdges& ed, const double* Tp, bool keep, double* parte, int tid) {
    for (int e = tid; e < ((ed.E + 63) & ~63); e += T) {
        double c = 0;
        if (e < ed.E && ed.on(e))
            c = pg_edge_cost(Tp + (size_t)ed.i[e] * 7, Tp + (size_t)ed.j[e] * 7, ed.Z + (size_t)e * 7, ed.w + (size_t)e * 6, keep, ed.PQ + (size_t)e * 36,
                             ed.res + (size_t)e * 6);
        c = pg_wave_sum(c);
        if ((tid & 63) == 0) parte[e >> 6] = c;
    }
}

// a problem's stats and its status word (lane 0 writes)
template <class Stats>
PG_DEV void pg_write_stats(const Stats& st, int32_t* status, Stats* stats, int g, int tid) {
    if (tid == 0) { status[g] = st.status; if (stats) stats[g] = st; }
}

} // namespace
} // namespace vslam
