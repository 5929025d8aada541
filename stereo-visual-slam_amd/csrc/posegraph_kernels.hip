// posegraph_kernels.hip -- pose-graph optimisation (include/vslam_hip.h "pose-graph optimisation").
//
// One persistent workgroup of 256 lanes per graph runs every Levenberg-Marquardt iteration of its graph: linearise the edges, build the gradient and
// the diagonal blocks, solve (H + lambda diag(H)) delta = -g by preconditioned conjugate gradients that never form H (edge phase t_e = W (J_i p_i +
// J_j p_j), node phase y_n = sum J' t_e + lambda D p_n), try the step, accept or reject.  No grid-wide synchronisation, no host round trip.
// The set-up phases and the edge cost pass this solver shares with full BA are in pg_solver.h.
//
// A Jacobian A Ad(T) has the block form [[P, Q], [0, P]] (A = [[a, b], [0, a]], Ad = [[R, t^R], [0, R]]), so an edge stores 4 x 9 doubles, not 2 x 36.
//
// Determinism.  A lane takes the indices tid, tid + 256, ... of every loop, so index k always sits in lane k % 64 of some wave.  A sum over indices
// is (1) an xor butterfly over the 64 indices of an aligned block, (2) the block sums added in ascending order by every lane.  Neither depends on the
// workgroup width or on the other graphs.  Node sums walk the node's incidence list, which is sorted by edge.  The only atomics are integer.
//
// The chain preconditioner is a block LDL' of the block-tridiagonal M: S_k = M_kk - W_k O_{k-1}, W_k = O_{k-1}' S_{k-1}^-1, F_k = S_k^-1, so that
// M^-1 r is u_k = r_k - W_k u_{k-1} upwards and z_k = F_k u_k - W_{k+1}' z_{k+1} downwards: N dependent 6 x 6 steps each way, on six lanes of wave 0
// (lane = matrix row, the vector of the previous step passed through v_readlane; the loads of eight steps are issued together, since only the
// arithmetic of a step depends on the step before it).
#include <algorithm>

#include "pg_solver.h"
#include "se3_device.h"
#include "vslam_internal.h"

namespace vslam {

constexpr int kPgThreads = 256;
constexpr int kPgChainMaxLoops = 16;   // pg_precond = -1: the chain preconditioner up to this many edges off the chain
constexpr int kPgChunk = 8;   // steps of the chain sweeps whose loads are in flight together

struct PgState {
    int32_t* status;                             // n_graphs (first slot: vslam_pose_graph_status_dev reads it)
    double *PQ, *res, *te;                       // per edge: Pi Qi Pj Qj (36), residual (6), W J p (6)
    double *H, *O, *F, *W;                       // per node: diagonal block of H, block (k, k + 1) of H, and the preconditioner's F_k, W_k (36 each)
    double *b, *x, *r, *z, *p, *y, *u, *D;       // per node, 6 each
    double* Tnew;                                // per node, 7: the candidate poses
    int32_t *held, *start, *cursor, *inc;        // per node: held flag, incidence offsets (N + 1 per graph), fill cursor; per edge x 2: 2 e + side
    double *part0, *part1, *part2, *parte;       // block sums: three per 64 nodes, one per 64 edges
};

struct PgArgs {
    vslam_pose_graph g;
    vslam_pose_graph_params p;
    int precond;
    double* T_out;
    vslam_pose_graph_stats* stats;
    PgState s;
};

__global__ __launch_bounds__(kPgThreads) void pose_graph_kernel(PgArgs a) {
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    constexpr int T = kPgThreads;
    const PgState& s = a.s;
    __shared__ int sh_scan[T];
    __shared__ int sh_cnt[4];   // free nodes, edges off the chain, singular flag, spare

    // ---- the graph's ranges
    const int G = a.g.n_graphs;
    const int n0 = a.g.d_node_off[g], n1 = a.g.d_node_off[g + 1], e0 = a.g.d_edge_off[g], e1 = a.g.d_edge_off[g + 1];
    const int ok = __syncthreads_and(pg_own_range<T>(a.g.d_node_off, G, g, a.g.total_nodes, tid) & pg_own_range<T>(a.g.d_edge_off, G, g, a.g.total_edges, tid));
    vslam_pose_graph_stats st;
    st.chi2_init = st.chi2_final = 0; st.lambda = a.p.lambda_init; st.lm_iters = st.pcg_iters = st.n_free = 0; st.status = 0;
    if (!ok) {
        st.status = VSLAM_PG_BAD_INDEX;
        pg_write_stats(st, s.status, a.stats, g, tid);
        return;
    }
    const int N = n1 - n0, E = e1 - e0;
    const PgEdges ed = {E, a.g.d_edge_i + e0, a.g.d_edge_j + e0, a.g.d_edge_Z + (size_t)e0 * 7, a.g.d_edge_w + (size_t)e0 * 6,
                        a.g.d_edge_active ? a.g.d_edge_active + e0 : nullptr, s.PQ + (size_t)e0 * 36, s.res + (size_t)e0 * 6};
    const double* Tin = a.g.d_T + (size_t)n0 * 7;
    double* To = a.T_out + (size_t)n0 * 7;
    double* te = s.te + (size_t)e0 * 6;
    double* Hd = s.H + (size_t)n0 * 36; double* Od = s.O + (size_t)n0 * 36; double* Fd = s.F + (size_t)n0 * 36; double* Wd = s.W + (size_t)n0 * 36;
    double* vb = s.b + (size_t)n0 * 6; double* vx = s.x + (size_t)n0 * 6; double* vr = s.r + (size_t)n0 * 6; double* vz = s.z + (size_t)n0 * 6;
    double* vp = s.p + (size_t)n0 * 6; double* vy = s.y + (size_t)n0 * 6; double* vu = s.u + (size_t)n0 * 6; double* vD = s.D + (size_t)n0 * 6;
    double* Tn = s.Tnew + (size_t)n0 * 7;
    int32_t* held = s.held + n0; int32_t* start = s.start + n0 + g; int32_t* cursor = s.cursor + n0; int32_t* inc = s.inc + (size_t)e0 * 2;
    double* part0 = s.part0 + (n0 >> 6) + g; double* part1 = s.part1 + (n0 >> 6) + g; double* part2 = s.part2 + (n0 >> 6) + g;
    double* parte = s.parte + (e0 >> 6) + g;
    const int Nr = (N + 63) & ~63;

    // ---- the caller's ids and values; poses are copied through
    int bad = 0, nonfinite = 0;
    pg_check_edges<T>(ed, N, tid, bad, nonfinite);
    pg_copy_poses<T>(Tin, To, N, tid, nonfinite);
    bad = __syncthreads_or(bad);
    nonfinite = __syncthreads_or(nonfinite);
    if (bad || nonfinite) {
        st.status = (bad ? VSLAM_PG_BAD_INDEX : 0) | (nonfinite ? VSLAM_PG_NONFINITE : 0);
        pg_write_stats(st, s.status, a.stats, g, tid);
        return;
    }

    // ---- held nodes and the incidence lists (CSR over the active edges, each list ascending by edge)
    if (tid < 4) sh_cnt[tid] = 0;
    for (int k = tid; k < N; k += T) { held[k] = a.g.d_fixed ? (a.g.d_fixed[n0 + k] != 0) : (k == 0); cursor[k] = 0; }
    __syncthreads();
    {
        int off_chain = 0;
        for (int e = tid; e < E; e += T) {
            if (!ed.on(e)) continue;
            atomicAdd(&cursor[ed.i[e]], 1); atomicAdd(&cursor[ed.j[e]], 1);
            const int d = ed.i[e] - ed.j[e];
            off_chain += (d != 1 && d != -1);
        }
        if (off_chain) atomicAdd(&sh_cnt[1], off_chain);
    }
    __syncthreads();
    pg_hold_isolated<T>(held, N, tid, &sh_cnt[0], [&](int k) { return cursor[k] == 0; });
    pg_counts_to_offsets<T>(cursor, start, N, sh_scan, tid);
    for (int e = tid; e < E; e += T) {
        if (!ed.on(e)) continue;
        inc[atomicAdd(&cursor[ed.i[e]], 1)] = 2 * e;
        inc[atomicAdd(&cursor[ed.j[e]], 1)] = 2 * e + 1;
    }
    __syncthreads();
    pg_sort_lists_by_lane<T>(start, inc, N, tid);
    for (int k = tid; k < N; k += T) {
        for (int q = 0; q < 6; ++q) {
            const size_t o = (size_t)k * 6 + q;
            vb[o] = vx[o] = vr[o] = vz[o] = vp[o] = vy[o] = vu[o] = vD[o] = 0.0;
        }
    }
    __syncthreads();
    const int n_free = sh_cnt[0], n_loop = sh_cnt[1];
    st.n_free = n_free;
    // the library's rule (profiles/pose_graph.json): with 5 edges off the chain the chain preconditioner was 1.3 - 5 x faster at 64,
    // 512 and 4096 nodes, with 64 block-Jacobi was 1.6 - 4 x faster at 64 and 512; the sweep has no point in between, the threshold is their geometric mean
    const int precond = a.precond >= 0 ? a.precond : (n_loop <= kPgChainMaxLoops ? 1 : 0);

    // the cost of the active edges at poses Tp; with `lin` the residuals and Jacobians are kept for the solver
    auto cost_of = [&](const double* Tp, bool lin) -> double {
        pg_edge_cost_pass<T>(ed, Tp, lin, parte, tid);
        __syncthreads();
        const double total = pg_sum_parts(parte, E);
        __syncthreads();   // (parte is free again)
        return total;
    };

    double cost = cost_of(To, true);
    st.chi2_init = st.chi2_final = cost;
    double lambda = a.p.lambda_init;
    bool fresh = true;   // the linearisation in PQ / res belongs to To and the gradient has not been built from it yet
    int status = 0;
    const int max_iters = n_free > 0 ? a.p.max_iters : 0;

    for (int it = 0; it < max_iters; ++it) {
        if (fresh) {
            // ---- gradient b = -sum J' W r, diagonal blocks H_kk = sum J' W J and the blocks (k, k + 1) of the chain edges
            for (int k = tid; k < N; k += T) {
                double Hk[36], Ok[36], bk[6];
#pragma unroll
                for (int q = 0; q < 36; ++q) { Hk[q] = 0; Ok[q] = 0; }
#pragma unroll
                for (int q = 0; q < 6; ++q) bk[q] = 0;
                if (held[k]) {
                    Hk[0] = Hk[7] = Hk[14] = Hk[21] = Hk[28] = Hk[35] = 1.0;
                } else {
                    const bool next_free = k + 1 < N && !held[k + 1];
                    for (int q = start[k]; q < start[k + 1]; ++q) {
                        const int e = inc[q] >> 1, side = inc[q] & 1;
                        const double* pq = ed.PQ + (size_t)e * 36;
                        double Pa[9], Qa[9], w[6], wr[6], o[6];
#pragma unroll
                        for (int m = 0; m < 9; ++m) { Pa[m] = pq[side * 18 + m]; Qa[m] = pq[side * 18 + 9 + m]; }
#pragma unroll
                        for (int m = 0; m < 6; ++m) { w[m] = ed.w[(size_t)e * 6 + m]; wr[m] = w[m] * ed.res[(size_t)e * 6 + m]; }
                        pg_JT(Pa, Qa, wr, o);
#pragma unroll
                        for (int m = 0; m < 6; ++m) bk[m] -= o[m];
                        pg_JtWJ(Pa, Qa, Pa, Qa, w, Hk);
                        const int other = side ? ed.i[e] : ed.j[e];
                        if (next_free && other == k + 1) {
                            double Pb[9], Qb[9];
#pragma unroll
                            for (int m = 0; m < 9; ++m) { Pb[m] = pq[(1 - side) * 18 + m]; Qb[m] = pq[(1 - side) * 18 + 9 + m]; }
                            pg_JtWJ(Pa, Qa, Pb, Qb, w, Ok);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 36; ++q) { Hd[(size_t)k * 36 + q] = Hk[q]; Od[(size_t)k * 36 + q] = Ok[q]; }
#pragma unroll
                for (int q = 0; q < 6; ++q) { vb[(size_t)k * 6 + q] = bk[q]; vD[(size_t)k * 6 + q] = held[k] ? 0.0 : Hk[q * 7]; }
            }
            fresh = false;
            __syncthreads();
        }

        // ---- the preconditioner of H + lambda diag(H)
        if (precond == 0) {
            int sing = 0;
            for (int k = tid; k < N; k += T) {
                if (held[k]) continue;
                double M[36];
#pragma unroll
                for (int q = 0; q < 36; ++q) M[q] = Hd[(size_t)k * 36 + q];
#pragma unroll
                for (int q = 0; q < 6; ++q) M[q * 7] += lambda * vD[(size_t)k * 6 + q];
                sing |= pg_inv6(M);
#pragma unroll
                for (int q = 0; q < 36; ++q) Fd[(size_t)k * 36 + q] = M[q];
            }
            if (sing) atomicOr(&sh_cnt[2], 1);
        } else if (tid < 64) {
            const int row = lane < 6 ? lane : 0;
            double Wrow[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) Wrow[c] = 0;
            bool sing = false;
            for (int k = 0; k < N; ++k) {
                double S[6];
                const double dk = lambda * vD[(size_t)k * 6 + row];
#pragma unroll
                for (int c = 0; c < 6; ++c) S[c] = Hd[(size_t)k * 36 + row * 6 + c] + (c == row ? dk : 0.0);
                if (k > 0) {
                    const double* Op = Od + (size_t)(k - 1) * 36;
#pragma unroll
                    for (int c = 0; c < 6; ++c)
#pragma unroll
                        for (int m = 0; m < 6; ++m) S[c] -= Wrow[m] * Op[m * 6 + c];
                }
                if (lane < 6) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) Wd[(size_t)k * 36 + row * 6 + c] = Wrow[c];
                }
                sing |= pg_inv6_rows(S, row);
                if (lane < 6) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) Fd[(size_t)k * 36 + row * 6 + c] = S[c];
                }
                // W_{k+1} = O_k' F_k: row `row` is sum_m O_k[m][row] F_k[m][.]
                double Wn[6];
#pragma unroll
                for (int c = 0; c < 6; ++c) Wn[c] = 0;
#pragma unroll
                for (int m = 0; m < 6; ++m) {
                    const double o = Od[(size_t)k * 36 + m * 6 + row];
#pragma unroll
                    for (int c = 0; c < 6; ++c) Wn[c] += o * pg_readlane(S[c], m);
                }
#pragma unroll
                for (int c = 0; c < 6; ++c) Wrow[c] = Wn[c];
            }
            if (sing && lane == 0) atomicOr(&sh_cnt[2], 1);
        }
        __syncthreads();

        // z = M^-1 r and the block sums of r.z (part1) and r.r (part2)
        auto precondition = [&]() {
            if (precond == 0) {
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
                    if (lane == 0) { part1[k >> 6] = rz; part2[k >> 6] = rr; }
                }
            } else {
                __syncthreads();   // (r of every node is written)
                if (tid < 64) {
                    // The loads of a step do not depend on the step before it, only the arithmetic does: the loads of kPgChunk steps are issued
                    // together and the steps then run from registers, so a chunk pays one memory round trip instead of kPgChunk.
                    const int row = lane < 6 ? lane : 0;
                    double prev[6];
#pragma unroll
                    for (int c = 0; c < 6; ++c) prev[c] = 0;
                    for (int k0 = 0; k0 < N; k0 += kPgChunk) {
                        double Wc[kPgChunk][6], rc[kPgChunk];
#pragma unroll
                        for (int m = 0; m < kPgChunk; ++m) {
                            const int k = min(k0 + m, N - 1);
                            rc[m] = vr[(size_t)k * 6 + row];
#pragma unroll
                            for (int c = 0; c < 6; ++c) Wc[m][c] = Wd[(size_t)k * 36 + row * 6 + c];
                        }
#pragma unroll
                        for (int m = 0; m < kPgChunk; ++m) {
                            if (k0 + m < N) {
                                double acc = rc[m];
#pragma unroll
                                for (int c = 0; c < 6; ++c) acc -= Wc[m][c] * prev[c];
                                if (lane < 6) vu[(size_t)(k0 + m) * 6 + row] = acc;
#pragma unroll
                                for (int c = 0; c < 6; ++c) prev[c] = pg_readlane(acc, c);
                            }
                        }
                    }
                    __threadfence_block();
#pragma unroll
                    for (int c = 0; c < 6; ++c) prev[c] = 0;
                    for (int k0 = N - 1; k0 >= 0; k0 -= kPgChunk) {
                        double Fu[kPgChunk], Wc[kPgChunk][6];   // (F_k u_k does not depend on the recurrence either)
#pragma unroll
                        for (int m = 0; m < kPgChunk; ++m) {
                            const int k = max(k0 - m, 0);
                            double acc = 0;
#pragma unroll
                            for (int c = 0; c < 6; ++c) acc += Fd[(size_t)k * 36 + row * 6 + c] * vu[(size_t)k * 6 + c];
                            Fu[m] = acc;
#pragma unroll
                            for (int c = 0; c < 6; ++c) Wc[m][c] = k + 1 < N ? Wd[(size_t)(k + 1) * 36 + c * 6 + row] : 0.0;
                        }
#pragma unroll
                        for (int m = 0; m < kPgChunk; ++m) {
                            if (k0 - m >= 0) {
                                double acc = Fu[m];
#pragma unroll
                                for (int c = 0; c < 6; ++c) acc -= Wc[m][c] * prev[c];
                                if (lane < 6) vz[(size_t)(k0 - m) * 6 + row] = acc;
#pragma unroll
                                for (int c = 0; c < 6; ++c) prev[c] = pg_readlane(acc, c);
                            }
                        }
                    }
                }
                __syncthreads();
                for (int k = tid; k < Nr; k += T) {
                    double rz = 0, rr = 0;
                    if (k < N && !held[k]) {
#pragma unroll
                        for (int q = 0; q < 6; ++q) { const double rq = vr[(size_t)k * 6 + q]; rz += rq * vz[(size_t)k * 6 + q]; rr += rq * rq; }
                    }
                    rz = pg_wave_sum(rz); rr = pg_wave_sum(rr);
                    if (lane == 0) { part1[k >> 6] = rz; part2[k >> 6] = rr; }
                }
            }
            __syncthreads();
        };

        // ---- conjugate gradients on (H + lambda D) x = b, x0 = 0
        for (int k = tid; k < N; k += T) {
#pragma unroll
            for (int q = 0; q < 6; ++q) { vx[(size_t)k * 6 + q] = 0.0; vr[(size_t)k * 6 + q] = vb[(size_t)k * 6 + q]; }
        }
        precondition();
        double rz = pg_sum_parts(part1, N), rr = pg_sum_parts(part2, N);
        const double rr0 = rr;
        for (int k = tid; k < N; k += T) {
#pragma unroll
            for (int q = 0; q < 6; ++q) vp[(size_t)k * 6 + q] = vz[(size_t)k * 6 + q];
        }
        __syncthreads();
        int cg = 0;
        const double tol2 = a.p.pcg_tol * a.p.pcg_tol;
        while (rr0 > 0 && rr > tol2 * rr0) {
            if (cg >= a.p.pcg_max_iters) { status |= VSLAM_PG_PCG_CAP; break; }
            // edge phase: t_e = W (J_i p_i + J_j p_j)
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
                for (int m = 0; m < 6; ++m) te[(size_t)e * 6 + m] = ed.w[(size_t)e * 6 + m] * (t1[m] + t2[m]);
            }
            __syncthreads();
            // node phase: y_n = sum J' t_e + lambda D p_n, and the block sums of p.y
            for (int k = tid; k < Nr; k += T) {
                double py = 0;
                if (k < N && !held[k]) {
                    double yk[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) yk[q] = lambda * vD[(size_t)k * 6 + q] * vp[(size_t)k * 6 + q];
                    for (int q = start[k]; q < start[k + 1]; ++q) {
                        const int e = inc[q] >> 1, side = inc[q] & 1;
                        const double* pq = ed.PQ + (size_t)e * 36 + side * 18;
                        double Pm[9], Qm[9], t[6], o[6];
#pragma unroll
                        for (int m = 0; m < 9; ++m) { Pm[m] = pq[m]; Qm[m] = pq[9 + m]; }
#pragma unroll
                        for (int m = 0; m < 6; ++m) t[m] = te[(size_t)e * 6 + m];
                        pg_JT(Pm, Qm, t, o);
#pragma unroll
                        for (int m = 0; m < 6; ++m) yk[m] += o[m];
                    }
#pragma unroll
                    for (int q = 0; q < 6; ++q) { vy[(size_t)k * 6 + q] = yk[q]; py += vp[(size_t)k * 6 + q] * yk[q]; }
                }
                py = pg_wave_sum(py);
                if (lane == 0) part0[k >> 6] = py;
            }
            __syncthreads();
            const double py = pg_sum_parts(part0, N);
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
            const double rz_new = pg_sum_parts(part1, N);
            rr = pg_sum_parts(part2, N);
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

        // ---- the candidate T' = exp(x) T and |x|
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
            if (lane == 0) part0[k >> 6] = dd;
        }
        __syncthreads();
        const double step = sqrt(pg_sum_parts(part0, N));
        const double cost_new = cost_of(Tn, false);
        st.lm_iters = it + 1;
        if (cost_new < cost) {   // (false for a NaN)
            for (int k = tid; k < N; k += T) {
#pragma unroll
                for (int q = 0; q < 7; ++q) To[(size_t)k * 7 + q] = Tn[(size_t)k * 7 + q];
            }
            __syncthreads();
            cost = cost_of(To, true);   // (the same sum as cost_new, and the linearisation of the next iteration)
            fresh = true;
            lambda = fmax(lambda / 10.0, 1e-12);
        } else {
            lambda *= 10.0;
        }
        if (!(step >= a.p.step_tol)) break;
        if (lambda > 1e12) { status |= VSLAM_PG_LAMBDA; break; }
    }

    // ---- per-edge chi2 of every edge at the output poses
    if (a.g.d_edge_chi2) {
        for (int e = tid; e < E; e += T) {
            const int i = ed.i[e], j = ed.j[e];
            double Ti[7], Tj[7], Z[7], w[6], r[6], Ee[7], Zi[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) { Ti[q] = To[(size_t)i * 7 + q]; Tj[q] = To[(size_t)j * 7 + q]; Z[q] = ed.Z[(size_t)e * 7 + q]; }
#pragma unroll
            for (int q = 0; q < 6; ++q) w[q] = ed.w[(size_t)e * 6 + q];
            pg_residual(Ti, Tj, Z, r, Ee, Zi);
            a.g.d_edge_chi2[e0 + e] = pg_chi2(r, w);
        }
    }
    if (tid == 0) {
        st.chi2_final = cost; st.lambda = lambda;
        st.status = status | (sh_cnt[2] ? VSLAM_PG_SINGULAR : 0);
        s.status[g] = st.status;
        if (a.stats) a.stats[g] = st;
    }
}

int launch_pose_graph(const vslam_pose_graph& g, const vslam_pose_graph_params& p, int precond, double* d_T_out, vslam_pose_graph_stats* d_stats, DevBuf& buf,
                      hipStream_t stream) {
    PgArgs a;
    a.g = g; a.p = p; a.precond = precond; a.T_out = d_T_out; a.stats = d_stats;
    const size_t G = (size_t)g.n_graphs, N = (size_t)g.total_nodes, E = (size_t)g.total_edges;
    PgState& s = a.s;
    if (int rc = carve(buf, stream, [&](Layout& l) {
            s.status = l.take<int32_t>(G);
            s.PQ = l.take<double>(E * 36); s.res = l.take<double>(E * 6); s.te = l.take<double>(E * 6);
            s.H = l.take<double>(N * 36); s.O = l.take<double>(N * 36); s.F = l.take<double>(N * 36); s.W = l.take<double>(N * 36);
            s.b = l.take<double>(N * 6); s.x = l.take<double>(N * 6); s.r = l.take<double>(N * 6); s.z = l.take<double>(N * 6);
            s.p = l.take<double>(N * 6); s.y = l.take<double>(N * 6); s.u = l.take<double>(N * 6); s.D = l.take<double>(N * 6);
            s.Tnew = l.take<double>(N * 7);
            s.held = l.take<int32_t>(N); s.start = l.take<int32_t>(N + G); s.cursor = l.take<int32_t>(N); s.inc = l.take<int32_t>(E * 2);
            s.part0 = l.take<double>(N / 64 + G + 1); s.part1 = l.take<double>(N / 64 + G + 1); s.part2 = l.take<double>(N / 64 + G + 1);
            s.parte = l.take<double>(E / 64 + G + 1);
        })) return rc;
    if (g.n_graphs == 0) return VSLAM_OK;
    ProfScope prof__(stream, "pose_graph_kernel");
    hipLaunchKernelGGL(pose_graph_kernel, dim3(g.n_graphs), dim3(kPgThreads), 0, stream, a);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
