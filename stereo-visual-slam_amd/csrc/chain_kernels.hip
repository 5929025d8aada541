// chain_kernels.hip -- the chained BA of throughput mode (vslam_ba_chain_dev): the windows of a sequence run one after another, each from the poses and
// is_inlier flags the previous one left, and the sequences of a batch run side by side.  Step j stages window first[s] + j of every sequence s that
// has one into a batch of its own, the BA schedule runs on that batch (launch_lm_windows, untouched), and the results go back to the caller's arrays
// and into the chain state.  Three kernels per step, all copies: chain_offsets_kernel, chain_gather_kernel, chain_scatter_kernel.
// What a window hands to the next (optimization.cpp:160, :272-278; optimize_map never moves a landmark): the poses of the keyframes they share and one
// is_inlier byte per landmark.  A keyframe is its batch frame index, a landmark the root of its track (vslam_set_window_ids).
#include "vslam_internal.h"

namespace vslam {

constexpr int kChainBlock = 256;
constexpr int kChainSlices = 8; // workgroups per window of the gather / scatter kernels (a window: a few thousand landmarks and edges)

// inclusive scan of `v` over the 256 lanes of the workgroup; *total = the workgroup's sum.  red: 4 ints of LDS.
__device__ inline int chain_block_scan(int v, int* red, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o); if (lane >= o) v += t; }
    __syncthreads(); // (red may still be read from the previous call)
    if (lane == 63) red[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < 4; ++k) { const int t = red[k]; all += t; if (k < wave) before += t; }
    *total = all;
    return v + before;
}

// What window w brings to its step: is it active (d_n_kf[w] >= min_kf and offsets that lie inside the caller's arrays), and its landmark / edge counts.
struct ChainWin { int nk, n_lm, n_edge; bool active; };
__device__ inline ChainWin chain_window(const ChainArgs& a, int w) {
    ChainWin c;
    const int nk = a.n_kf_w ? a.n_kf_w[w] : a.n_kf;
    c.nk = nk < 0 ? 0 : (nk > a.n_kf ? a.n_kf : nk);
    const long long l0 = a.lm_off[w], l1 = a.lm_off[w + 1], e0 = a.edge_off[w], e1 = a.edge_off[w + 1];
    const bool in_range = l0 >= 0 && l1 >= l0 && l1 <= a.total_lm && e0 >= 0 && e1 >= e0 && e1 <= a.total_edge;
    c.n_lm = in_range ? (int)(l1 - l0) : 0; c.n_edge = in_range ? (int)(e1 - e0) : 0;
    c.active = in_range && c.nk >= 1 && c.nk >= a.min_kf;
    return c;
}

// the frame slot k of window w holds: the caller's set, or the sliding window [max(start(w), w - n_kf + 1), w]; -1 for "none" (out of range included)
__device__ inline int chain_frame(const ChainArgs& a, int w, int k, int seg_start) {
    int g;
    if (a.kf_frame) g = a.kf_frame[(size_t)w * a.n_kf + k];
    else { const int lo = w - a.n_kf + 1; g = (lo > seg_start ? lo : seg_start) + k; }
    return (g >= 0 && g < a.n_windows) ? g : -1;
}

// ---- one workgroup: the staging batch's offsets.  Slot i = the i-th sequence (ascending) with more than `step` frames, its window w = first[s] + step;
// an inactive window is EMPTY (offsets do not advance, n_kf 0).  A step whose windows would not fit the staging arrays (offsets that overlap: not a
// builder's output) runs with every window inactive.
__global__ __launch_bounds__(kChainBlock) void chain_offsets_kernel(ChainArgs a, int step) {
    __shared__ int red[4];
    const int tid = threadIdx.x;
    long long sum_lm = 0, sum_edge = 0; // (phase 1: do the active windows fit?  64-bit: the sums of overlapping ranges can pass 2^31)
    for (int s = tid; s < a.n_seg; s += kChainBlock) {
        const int f0 = a.first ? a.first[s] : 0, f1 = a.first ? a.first[s + 1] : a.n_windows;
        if (f1 - f0 > step && f0 + step < a.n_windows && f0 >= 0) { const ChainWin c = chain_window(a, f0 + step); if (c.active) { sum_lm += c.n_lm; sum_edge += c.n_edge; } }
    }
    __shared__ long long tot[2][kChainBlock / 64];
    for (int o = 32; o > 0; o >>= 1) { sum_lm += __shfl_xor(sum_lm, o); sum_edge += __shfl_xor(sum_edge, o); }
    if ((tid & 63) == 0) { tot[0][tid >> 6] = sum_lm; tot[1][tid >> 6] = sum_edge; }
    __syncthreads();
    long long all_lm = 0, all_edge = 0;
    for (int k = 0; k < kChainBlock / 64; ++k) { all_lm += tot[0][k]; all_edge += tot[1][k]; }
    const bool fits = all_lm <= a.total_lm && all_edge <= a.total_edge;
    int slot0 = 0, lm0 = 0, edge0 = 0;
    for (int base = 0; base < a.n_seg; base += kChainBlock) { // (uniform trip count: the scans hold barriers)
        const int s = base + tid;
        int live = 0, n_lm = 0, n_edge = 0, nk = 0, w = 0;
        if (s < a.n_seg) {
            const int f0 = a.first ? a.first[s] : 0, f1 = a.first ? a.first[s + 1] : a.n_windows;
            if (f1 - f0 > step && f0 + step < a.n_windows && f0 >= 0) {
                live = 1; w = f0 + step;
                const ChainWin c = chain_window(a, w);
                if (c.active && fits) { n_lm = c.n_lm; n_edge = c.n_edge; nk = c.nk; }
            }
        }
        int t_slot, t_lm, t_edge;
        const int i_slot = chain_block_scan(live, red, &t_slot), i_lm = chain_block_scan(n_lm, red, &t_lm), i_edge = chain_block_scan(n_edge, red, &t_edge);
        if (live) {
            const int i = slot0 + i_slot - 1;
            a.s_win[i] = w; a.s_n_kf[i] = nk; a.s_lm_off[i] = lm0 + i_lm - n_lm; a.s_edge_off[i] = edge0 + i_edge - n_edge;
        }
        slot0 += t_slot; lm0 += t_lm; edge0 += t_edge;
    }
    if (tid == 0) { a.s_lm_off[slot0] = lm0; a.s_edge_off[slot0] = edge0; }
}

// n 32-bit words, lane t of nt: 16 bytes per lane where source and destination share their alignment (window offsets that agree modulo 4 words)
__device__ inline void chain_copy_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int n, int t, int nt) {
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), sa = reinterpret_cast<uintptr_t>(src);
    if (((da ^ sa) & 15) != 0) { for (int i = t; i < n; i += nt) dst[i] = src[i]; return; }
    int head = (int)(((16 - (da & 15)) & 15) >> 2);
    if (head > n) head = n;
    const int body = (n - head) >> 2, tail = head + (body << 2);
    if (t < head) dst[t] = src[t];
    const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    for (int i = t; i < body; i += nt) d4[i] = s4[i];
    for (int i = tail + t; i < n; i += nt) dst[i] = src[i];
}

// ---- grid (slots, kChainSlices): slot i's window into the staging batch, with the chain's poses and flags substituted (the entry state).
// An inactive window that holds keyframes passes the carried poses and flags through to the caller's arrays and enters its own pose into the state.
__global__ __launch_bounds__(kChainBlock) void chain_gather_kernel(ChainArgs a) {
    const int i = blockIdx.x, w = a.s_win[i], tid = threadIdx.x;
    const int t = blockIdx.y * kChainBlock + tid, nt = gridDim.y * kChainBlock;
    const ChainWin c = chain_window(a, w);
    const bool active = a.s_n_kf[i] > 0; // (the offsets kernel's verdict: chain_window's, and the step fits)
    const int l_src = a.lm_off[w], l_dst = a.s_lm_off[i];
    if (blockIdx.y == 0) {
        if (tid == 0 && a.ran) a.ran[w] = active ? 1 : 0;
        int seg_start = 0;
        if (!a.kf_frame && a.first) { // (the sliding window restarts at the segment's first frame)
            int lo = 0, hi = a.n_seg;
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.first[mid] <= w) lo = mid; else hi = mid; }
            seg_start = a.first[lo];
        }
        double* Tw = a.T + (size_t)w * a.n_kf * 7;
        double* Ts = a.s_T + (size_t)i * a.n_kf * 7;
        for (int e = tid; e < a.n_kf * 7; e += kChainBlock) {
            const int k = e / 7, comp = e - 7 * k;
            const double own = Tw[e];
            double v = own;
            if (k < c.nk) {
                const int g = chain_frame(a, w, k, seg_start);
                if (g == w) { if (!active) { a.pose[(size_t)w * 7 + comp] = own; if (comp == 0) a.pose_set[w] = 1; } }
                else if (g >= 0 && a.pose_set[g]) { v = a.pose[(size_t)g * 7 + comp]; if (!active) Tw[e] = v; }
            }
            Ts[e] = active ? v : own; // (an empty window: the builder's poses, slot 0 = the window's own)
        }
    }
    if (!active) { // pass-through of the flags (a window without keyframes is left as built)
        if (c.nk > 0)
            for (int l = t; l < c.n_lm; l += nt) {
                const int id = a.lm_id[l_src + l];
                a.lm_inlier[l_src + l] = (id >= 0 && id < a.n_roots) ? a.bit[id] : (uint8_t)1;
            }
        return;
    }
    for (int l = t; l < c.n_lm; l += nt) {
        const int id = a.lm_id[l_src + l];
        a.s_inl[l_dst + l] = (id >= 0 && id < a.n_roots) ? a.bit[id] : (uint8_t)1;
        if (a.s_rel) a.s_rel[l_dst + l] = a.reliable[l_src + l];
    }
    const int e_src = a.edge_off[w], e_dst = a.s_edge_off[i];
    chain_copy_words(reinterpret_cast<uint32_t*>(a.s_xyz + 3 * (size_t)l_dst), reinterpret_cast<const uint32_t*>(a.xyz + 3 * (size_t)l_src), 3 * c.n_lm, t, nt);
    chain_copy_words(reinterpret_cast<uint32_t*>(a.s_kf + e_dst), reinterpret_cast<const uint32_t*>(a.kf_idx + e_src), c.n_edge, t, nt);
    chain_copy_words(reinterpret_cast<uint32_t*>(a.s_lm + e_dst), reinterpret_cast<const uint32_t*>(a.lm_idx + e_src), c.n_edge, t, nt);
    chain_copy_words(reinterpret_cast<uint32_t*>(a.s_uv + 2 * (size_t)e_dst), reinterpret_cast<const uint32_t*>(a.uv + 2 * (size_t)e_src), 2 * c.n_edge, t, nt);
}

// ---- grid (slots, kChainSlices): an active window's results to the caller's arrays at window w and into the chain state
__global__ __launch_bounds__(kChainBlock) void chain_scatter_kernel(ChainArgs a, const int32_t* __restrict__ step_status) {
    const int i = blockIdx.x, w = a.s_win[i], tid = threadIdx.x;
    if (a.s_n_kf[i] <= 0) return;
    const int t = blockIdx.y * kChainBlock + tid, nt = gridDim.y * kChainBlock;
    const ChainWin c = chain_window(a, w);
    const int l_src = a.lm_off[w], l_dst = a.s_lm_off[i];
    if (blockIdx.y == 0) {
        if (tid == 0) a.status[w] = step_status[i];
        int seg_start = 0;
        if (!a.kf_frame && a.first) {
            int lo = 0, hi = a.n_seg;
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.first[mid] <= w) lo = mid; else hi = mid; }
            seg_start = a.first[lo];
        }
        double* Tw = a.T + (size_t)w * a.n_kf * 7;
        const double* Ts = a.s_T + (size_t)i * a.n_kf * 7;
        for (int e = tid; e < c.nk * 7; e += kChainBlock) {
            const int k = e / 7, comp = e - 7 * k;
            const double v = Ts[e];
            Tw[e] = v;
            const int g = chain_frame(a, w, k, seg_start);
            if (g >= 0) { a.pose[(size_t)g * 7 + comp] = v; if (comp == 0) a.pose_set[g] = 1; }
        }
        if (a.stats)
            chain_copy_words(reinterpret_cast<uint32_t*>(a.stats + w), reinterpret_cast<const uint32_t*>(a.s_stats + i), (int)(sizeof(vslam_lm_stats) / 4), tid, kChainBlock);
    }
    for (int l = t; l < c.n_lm; l += nt) {
        const uint8_t v = a.s_inl[l_dst + l];
        a.lm_inlier[l_src + l] = v;
        const int id = a.lm_id[l_src + l];
        if (id >= 0 && id < a.n_roots) a.bit[id] = v;
    }
    if (a.chi2) {
        const int e_src = a.edge_off[w], e_dst = a.s_edge_off[i];
        for (int e = t; e < c.n_edge; e += nt) a.chi2[e_src + e] = a.s_chi2[e_dst + e];
    }
}

int launch_chain_stage(const ChainArgs& a, int step, int n_slots, hipStream_t stream) {
    ProfScope prof__(stream, "ba_chain_kernels", 2);
    hipLaunchKernelGGL(chain_offsets_kernel, dim3(1), dim3(kChainBlock), 0, stream, a, step);
    hipLaunchKernelGGL(chain_gather_kernel, dim3(n_slots, kChainSlices), dim3(kChainBlock), 0, stream, a);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_chain_scatter(const ChainArgs& a, int n_slots, const int32_t* step_status, hipStream_t stream) {
    ProfScope prof__(stream, "ba_chain_kernels", 1);
    hipLaunchKernelGGL(chain_scatter_kernel, dim3(n_slots, kChainSlices), dim3(kChainBlock), 0, stream, a, step_status);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
