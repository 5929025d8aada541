// tsdf_dist_kernels.hip -- the surface map's clearance layer (include/vslam_hip.h "DISTANCE"): per voxel the squared Euclidean distance, in voxel
// units, to the nearest SITE of its map -- an occupied voxel with a free face neighbour -- up to a radius R <= 16 voxels, with the voxel's class, as
// one uint16 cell word; and point queries against it.  The layer is block-sparse with a key table of its own: it holds every claimed block of the
// pool and every block a site's ball can reach, most of which the pool never claimed.  Everything is an integer minimum over sites, so the layer
// depends neither on the order the blocks were claimed in nor on the form, and tests/tsdf_distance_ref.py restates it by brute force.
//
//   tsdf_dist_clear_kernel      the layer's keys empty, its masks, flags and counters zero
//   tsdf_dist_classify_kernel   one workgroup per claimed block of the pool, staged in LDS: the block claimed in the layer, its voxels classed, three
//                               512-bit masks (site, free, occupied) written by wave ballots, the sites counted, the blocks that hold one listed
//   tsdf_dist_dilate_kernel     one lane per (site block, offset within ceil(R / 8) blocks per axis): the block claimed in the layer if it is new
//   tsdf_dist_brute_kernel      (form 0) one workgroup per layer block, one lane per voxel: the minimum over the set bits of the site masks of the
//                               blocks around it, a block skipped when its nearest voxel is already too far
//   tsdf_dist_row_kernel        (form 1, pass x) per voxel the squared distance along x to the nearest site of its row within R
//   tsdf_dist_pass_kernel<a>    (form 1, passes y and z) min over |d| <= R of (the pass before at + d along the axis) + d^2; the last thresholds
//   tsdf_dist_counts_kernel     the three counts of a build
//   tsdf_dist_blocks_kernel     the layer's blocks by the emission rule, for readers and tests
//   tsdf_dist_query_kernel      one lane per point: index, one layer lookup, one uint16 load
// Claiming follows tsdf_claim: a relaxed key load, a compare-and-swap only on "empty", linear probing, no lane waits for another.  A block that
// finds no slot voids the whole layer (a flag the later kernels read; status bit 4).  Every cell has ONE owner lane: no atomics on the cells.
// Compiled with FMA contraction off (the Makefile's default); the only floating-point arithmetic is the query's.
#include "vslam_internal.h"

#include "tsdf_device.h"

namespace vslam {

constexpr uint32_t kDistNone = 0xFFFFu;     // an intermediate pass value: no site within reach along the axes done so far
constexpr uint32_t kDistFar = 0xFFFu;       // the cell word's d2 field: FAR
constexpr uint32_t kDistAbsent = 0xFFFFFFFFu;

// the layer's key table seen through the pool's lookup (tsdf_find reads keys and log2_blocks only)
__device__ __forceinline__ TsdfTable dist_keys(const TsdfLayer& L) {
    TsdfTable t;
    t.keys = L.keys; t.list = nullptr; t.pool = nullptr; t.counters = nullptr; t.frames = nullptr; t.pairs = nullptr;
    t.log2_blocks = L.log2_blocks; t.J = 0; t.frame_words = 0; t.vs = 0.f; t.inv = 0.f;
    return t;
}
__device__ __forceinline__ bool dist_in_range(int bx, int by, int bz) {
    return bx >= -kTsdfBHalf && bx < kTsdfBHalf && by >= -kTsdfBHalf && by < kTsdfBHalf && bz >= -kTsdfBHalf && bz < kTsdfBHalf;
}
__device__ __forceinline__ u64 dist_block_key(int map, int bx, int by, int bz) { // (in range)
    return (u64)(uint32_t)map << 45 | (u64)(uint32_t)(bx + kTsdfBHalf) << 30 | (u64)(uint32_t)(by + kTsdfBHalf) << 15 | (u64)(uint32_t)(bz + kTsdfBHalf);
}
// the layer slot of block (map, bx, by, bz), kDistAbsent if it is out of range or no slot holds it
__device__ __forceinline__ uint32_t dist_find(const TsdfLayer& L, int map, int bx, int by, int bz) {
    if (!dist_in_range(bx, by, bz)) return kDistAbsent;
    uint32_t s;
    return tsdf_find(dist_keys(L), dist_block_key(map, bx, by, bz), s) ? s : kDistAbsent;
}
// the slot that holds `key`, claimed if no slot held it; kDistAbsent (and the layer void) if the probe finds neither the key nor an empty slot
__device__ __forceinline__ uint32_t dist_claim(const TsdfLayer& L, unsigned long long* status, u64 key) {
    const TsdfTable kt = dist_keys(L);
    const uint32_t mask = (1u << L.log2_blocks) - 1u, probes = tsdf_probes(kt);
    uint32_t s = voxel_hash(key) & mask;
    for (uint32_t p = 0; p < probes; ++p, s = (s + 1) & mask) {
        u64 k = __hip_atomic_load(&L.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kVoxelEmpty) {
            k = atomicCAS(&L.keys[s], kVoxelEmpty, key);
            if (k == kVoxelEmpty) { // this lane claimed the slot: it enters the list (each slot is claimed once, so the list cannot overflow)
                const u64 i = atomicAdd(&L.counters[kDistNList], 1ull);
                L.list[i] = s;
                return s;
            }
        }
        if (k == key) return s;
    }
    atomicOr(&L.counters[kDistVoid], 1ull);
    atomicOr(status, 16ull);
    return kDistAbsent;
}

__global__ __launch_bounds__(kVoxelBlock) void tsdf_dist_clear_kernel(TsdfLayer L) {
    const size_t n_slots = (size_t)1 << L.log2_blocks, stride = (size_t)gridDim.x * kVoxelBlock, i0 = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x;
    for (size_t i = i0; i < n_slots; i += stride) { L.keys[i] = kVoxelEmpty; L.kind[i] = 0; }
    for (size_t i = i0; i < n_slots * kDistMaskWords; i += stride) L.masks[i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x < kDistCounters) L.counters[threadIdx.x] = 0ull;
}

// ------------------------------------------------------------------------------------------------------------------- classes and sites
// (38 VGPRs: eight waves per SIMD need <= 80 SGPRs on this device; the two tables and the neighbour lookups took 88 uncapped)
__global__ __launch_bounds__(kTsdfLanes) __attribute__((amdgpu_num_sgpr(72))) void tsdf_dist_classify_kernel(TsdfTable t, TsdfLayer L, int map_id, uint32_t min_w) {
    __shared__ uint4 lv[kTsdfLanes];
    __shared__ uint32_t sslot;
    const u64 n_list = t.counters[0];
    const int l = threadIdx.x, lane = l & 63, wave = l >> 6;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = t.list[i];
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        if (map_id >= 0 && id.map != map_id) continue; // (workgroup-uniform)
        __syncthreads(); // (the readers of the last block are done)
        const uint4 va = t.pool[(size_t)s * kTsdfLanes + l];
        lv[l] = va;
        if (l == 0) sslot = dist_claim(L, &t.counters[4], t.keys[s]);
        __syncthreads();
        const int ix = id.bx * 8 + (l & 7), iy = id.by * 8 + ((l >> 3) & 7), iz = id.bz * 8 + (l >> 6);
        const bool good = tsdf_good(va, min_w);
        const bool is_free = good && tsdf_num(va) > 0, occ = good && !is_free;
        bool site = false;
        if (occ) {
#pragma unroll 1
            for (int f = 0; f < 6 && !site; ++f) {
                const int d = (f & 1) ? 1 : -1, a = f >> 1;
                const uint4 vb = tsdf_fetch(t, lv, id, ix + (a == 0 ? d : 0), iy + (a == 1 ? d : 0), iz + (a == 2 ? d : 0));
                site = tsdf_good(vb, min_w) && tsdf_num(vb) > 0;
            }
        }
        const u64 b_site = __ballot(site), b_free = __ballot(is_free), b_occ = __ballot(occ);
        const int any_site = __syncthreads_or(site ? 1 : 0);
        const uint32_t ls = sslot;
        if (lane == 0) {
            if (b_site) atomicAdd(&L.counters[kDistSites], (u64)__popcll(b_site));
            if (ls != kDistAbsent) {
                u64* m = L.masks + (size_t)ls * kDistMaskWords;
                m[wave] = b_site; m[8 + wave] = b_free; m[16 + wave] = b_occ;
            }
        }
        if (l == 0 && ls != kDistAbsent) {
            L.kind[ls] = 1; // rule (a): claimed in the pool for a map the call covers
            if (any_site) { const u64 k = atomicAdd(&L.counters[kDistNSiteBlocks], 1ull); L.site_list[k] = ls; }
        }
    }
}

// every block within rb blocks per axis of a site block; a coordinate outside [-2^14, 2^14) drops the block.  The site block itself is there already.
// No merge of duplicates inside a wave: a block that is there already costs its lane one relaxed key load and no atomic, and the whole kernel
// takes 0.01 - 0.02 ms on the benchmark's maps, which a ballot-and-compare pass would not repay.
__global__ __launch_bounds__(kVoxelBlock) void tsdf_dist_dilate_kernel(TsdfLayer L, unsigned long long* status, int rb) {
    const int w = 2 * rb + 1, n_off = w * w * w;
    const u64 n = L.counters[kDistNSiteBlocks] * (u64)n_off;
    for (u64 it = (u64)blockIdx.x * kVoxelBlock + threadIdx.x; it < n; it += (u64)gridDim.x * kVoxelBlock) {
        const u64 i = it / (u64)n_off;
        const int o = (int)(it - i * (u64)n_off), ox = o % w - rb, oy = (o / w) % w - rb, oz = o / (w * w) - rb;
        if (ox == 0 && oy == 0 && oz == 0) continue;
        const TsdfBlockId id = tsdf_unpack(L.keys[L.site_list[i]]);
        const int bx = id.bx + ox, by = id.by + oy, bz = id.bz + oz;
        if (!dist_in_range(bx, by, bz)) continue;
        dist_claim(L, status, dist_block_key(id.map, bx, by, bz));
    }
}

// the cell word of the block's voxel l, the block's emission flag and the two block counts: the end of both forms (every lane of the workgroup calls it)
__device__ __forceinline__ void dist_finish(const TsdfLayer& L, uint32_t s, int l, uint32_t best, uint32_t R2) {
    const uint32_t d2 = best <= R2 ? best : kDistFar;
    const u64* m = L.masks + (size_t)s * kDistMaskWords;
    const int wave = l >> 6, lane = l & 63;
    const uint32_t cls = (uint32_t)((m[8 + wave] >> lane) & 1ull) | (uint32_t)((m[16 + wave] >> lane) & 1ull) << 1;
    L.cells[(size_t)s * kTsdfLanes + l] = (uint16_t)(d2 | cls << 12);
    const int near = __syncthreads_or(d2 != kDistFar ? 1 : 0);
    if (l == 0) {
        const uint8_t claimed = L.kind[s] & 1;
        if (near) L.kind[s] = claimed | 2; // rule (b): a voxel within R of a site
        if (claimed || near) atomicAdd(&L.counters[kDistNLayer], 1ull);
        if (!claimed && near) atomicAdd(&L.counters[kDistNKindB], 1ull);
    }
}

// ------------------------------------------------------------------------------------------------------------------- form 0
__global__ __launch_bounds__(kTsdfLanes) void tsdf_dist_brute_kernel(TsdfLayer L, int R, int rb) {
    if (L.counters[kDistVoid]) return;
    __shared__ uint32_t sslot;
    __shared__ u64 smask[8];
    const u64 n_list = L.counters[kDistNList];
    const int l = threadIdx.x, x = l & 7, y = (l >> 3) & 7, z = l >> 6, w = 2 * rb + 1;
    const uint32_t R2 = (uint32_t)(R * R);
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = L.list[i];
        const TsdfBlockId id = tsdf_unpack(L.keys[s]);
        uint32_t best = kDistNone;
        for (int o = 0; o < w * w * w; ++o) {
            const int ox = o % w - rb, oy = (o / w) % w - rb, oz = o / (w * w) - rb;
            // the nearest two voxels of the two blocks are 8 (|o| - 1) + 1 apart along an axis on which they differ
            const int gx = ox ? 8 * (abs(ox) - 1) + 1 : 0, gy = oy ? 8 * (abs(oy) - 1) + 1 : 0, gz = oz ? 8 * (abs(oz) - 1) + 1 : 0;
            if ((uint32_t)(gx * gx + gy * gy + gz * gz) > R2) continue; // (workgroup-uniform)
            __syncthreads(); // (the readers of the last neighbour are done)
            if (l == 0) sslot = dist_find(L, id.map, id.bx + ox, id.by + oy, id.bz + oz);
            __syncthreads();
            const uint32_t ns = sslot;
            if (ns == kDistAbsent) continue; // (workgroup-uniform)
            if (l < 8) smask[l] = L.masks[(size_t)ns * kDistMaskWords + l];
            __syncthreads();
            for (int wz = 0; wz < 8; ++wz) {
                u64 m = smask[wz];
                const int dz = oz * 8 + wz - z;
                while (m) {
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    const int dx = ox * 8 + (b & 7) - x, dy = oy * 8 + (b >> 3) - y;
                    const uint32_t d = (uint32_t)(dx * dx + dy * dy + dz * dz);
                    best = d < best ? d : best;
                }
            }
        }
        dist_finish(L, s, l, best, R2);
    }
}

// ------------------------------------------------------------------------------------------------------------------- form 1
// Pass x.  The site bits of the voxel's row over the 2 rb + 1 blocks along x, eight per block, as one word of at most 40 bits.
__global__ __launch_bounds__(kTsdfLanes) void tsdf_dist_row_kernel(TsdfLayer L, int R, int rb) {
    if (L.counters[kDistVoid]) return;
    __shared__ uint32_t sslot[5];
    __shared__ uint8_t srow[64 * 5];
    const u64 n_list = L.counters[kDistNList];
    const int l = threadIdx.x, x = l & 7, y = (l >> 3) & 7, z = l >> 6, w = 2 * rb + 1;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = L.list[i];
        const TsdfBlockId id = tsdf_unpack(L.keys[s]);
        __syncthreads(); // (the readers of the last block are done)
        if (l < w) sslot[l] = dist_find(L, id.map, id.bx + l - rb, id.by, id.bz);
        __syncthreads();
        if (x < w) {
            const uint32_t ns = sslot[x];
            srow[(z * 8 + y) * 5 + x] = ns == kDistAbsent ? (uint8_t)0 : (uint8_t)(L.masks[(size_t)ns * kDistMaskWords + z] >> (y * 8));
        }
        __syncthreads();
        u64 row = 0ull;
        for (int k = 0; k < w; ++k) row |= (u64)srow[(z * 8 + y) * 5 + k] << (8 * k);
        const int pos = rb * 8 + x; // (R <= 8 rb: pos - d >= 0 and pos + d < 8 w <= 40)
        uint32_t g = kDistNone;
        for (int d = 0; d <= R; ++d)
            if (((row >> (pos - d)) | (row >> (pos + d))) & 1ull) { g = (uint32_t)(d * d); break; }
        L.cells[(size_t)s * kTsdfLanes + l] = (uint16_t)g; // (scratch until the last pass writes the cell words)
    }
}

// Passes y (kAxis 1: pass x's values in L.cells -> L.tmp) and z (kAxis 2, the last: L.tmp -> thresholded and packed into L.cells; it reads no cell a
// neighbour writes).  The blocks along the axis are staged in LDS; one that the layer does not hold reads as "no site".
template <int kAxis>
__global__ __launch_bounds__(kTsdfLanes) void tsdf_dist_pass_kernel(TsdfLayer L, int R, int rb) {
    if (L.counters[kDistVoid]) return;
    constexpr bool kLast = kAxis == 2;
    __shared__ uint32_t sslot[5];
    __shared__ uint16_t sv[5 * kTsdfLanes];
    const uint16_t* src = kAxis == 1 ? L.cells : L.tmp;
    const u64 n_list = L.counters[kDistNList];
    const int l = threadIdx.x, w = 2 * rb + 1, sh = 3 * kAxis, c = (l >> sh) & 7, rest = l & ~(7 << sh);
    const uint32_t R2 = (uint32_t)(R * R);
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = L.list[i];
        const TsdfBlockId id = tsdf_unpack(L.keys[s]);
        __syncthreads(); // (the readers of the last block are done)
        if (l < w) sslot[l] = dist_find(L, id.map, id.bx, id.by + (kAxis == 1 ? l - rb : 0), id.bz + (kAxis == 2 ? l - rb : 0));
        __syncthreads();
        for (int k = 0; k < w; ++k) {
            const uint32_t ns = sslot[k];
            sv[k * kTsdfLanes + l] = ns == kDistAbsent ? (uint16_t)kDistNone : src[(size_t)ns * kTsdfLanes + l];
        }
        __syncthreads();
        const int pos = rb * 8 + c; // (R <= 8 rb: 0 <= pos + d < 8 w)
        uint32_t best = kDistNone;
        for (int d = -R; d <= R; ++d) {
            const int p = pos + d;
            const uint32_t v = sv[(p >> 3) * kTsdfLanes + (rest | (p & 7) << sh)];
            const uint32_t cand = v + (uint32_t)(d * d);
            best = (v != kDistNone && cand < best) ? cand : best;
        }
        if (kLast) dist_finish(L, s, l, best, R2);
        else L.tmp[(size_t)s * kTsdfLanes + l] = (uint16_t)best;
    }
}

__global__ void tsdf_dist_counts_kernel(TsdfLayer L, u64* __restrict__ counts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool ok = L.counters[kDistVoid] == 0ull;
    counts[0] = L.counters[kDistSites]; counts[1] = ok ? L.counters[kDistNLayer] : 0ull; counts[2] = ok ? L.counters[kDistNKindB] : 0ull;
}

// ------------------------------------------------------------------------------------------------------------------- readers
// the layer's blocks of map map_id (-1: all) by the emission rule: (map, bx, by, bz) and the block's 512 cell words; the counter runs on past `capacity`
__global__ __launch_bounds__(kTsdfLanes) void tsdf_dist_blocks_kernel(TsdfLayer L, int map_id, int32_t* __restrict__ block_out, uint16_t* __restrict__ cells_out, u64 capacity,
                                                                      u64* __restrict__ n_out) {
    if (L.counters[kDistVoid]) return; // a void layer serves nothing
    __shared__ u64 spos;
    const u64 n_list = L.counters[kDistNList];
    const int l = threadIdx.x;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = L.list[i];
        const TsdfBlockId id = tsdf_unpack(L.keys[s]);
        if ((map_id >= 0 && id.map != map_id) || L.kind[s] == 0) continue; // (workgroup-uniform)
        __syncthreads();
        if (l == 0) spos = atomicAdd(n_out, 1ull);
        __syncthreads();
        const u64 pos = spos;
        if (pos >= capacity) continue;
        cells_out[pos * kTsdfLanes + l] = L.cells[(size_t)s * kTsdfLanes + l];
        if (l == 0) reinterpret_cast<int4*>(block_out)[pos] = make_int4(id.map, id.bx, id.by, id.bz);
    }
}

__global__ __launch_bounds__(kVoxelBlock) void tsdf_dist_query_kernel(TsdfLayer L, double vs, const double* __restrict__ xyz, const int32_t* __restrict__ map_ids, u64 N,
                                                                      float* __restrict__ dist, uint8_t* __restrict__ cls_out) {
#pragma clang fp contract(off)
    const u64 n = (u64)blockIdx.x * kVoxelBlock + threadIdx.x;
    if (n >= N) return;
    const int m = map_ids[n];
    const double X0 = xyz[3 * n], X1 = xyz[3 * n + 1], X2 = xyz[3 * n + 2];
    const double i0 = floor(X0 / vs), i1 = floor(X1 / vs), i2 = floor(X2 / vs);
    const double lo = -(double)kVoxelHalf, hi = (double)kVoxelHalf;
    const bool valid = m >= 0 && m <= kVoxelMaxMap && isfinite(X0) && isfinite(X1) && isfinite(X2) &&
                       i0 >= lo && i0 < hi && i1 >= lo && i1 < hi && i2 >= lo && i2 < hi; // (a NaN index fails every comparison)
    if (!valid) { dist[n] = INFINITY; cls_out[n] = 3; return; }
    const int ix = (int)i0, iy = (int)i1, iz = (int)i2;
    uint32_t word = kDistFar; // a block outside the layer, or a void layer: FAR | UNKNOWN
    if (L.counters[kDistVoid] == 0ull) {
        const uint32_t s = dist_find(L, m, ix >> 3, iy >> 3, iz >> 3);
        if (s != kDistAbsent) word = L.cells[(size_t)s * kTsdfLanes + ((iz & 7) << 6 | (iy & 7) << 3 | (ix & 7))];
    }
    const uint32_t d2 = word & 0xFFFu, cls = (word >> 12) & 3u;
    float d;
    if (d2 == kDistFar) d = cls == 2u ? -INFINITY : INFINITY;
    else {
        d = (float)(sqrt((double)d2) * vs);
        if (cls == 2u && d2 > 0u) d = -d;
    }
    dist[n] = d; cls_out[n] = (uint8_t)cls;
}

// ------------------------------------------------------------------------------------------------------------------- launchers
size_t tsdf_dist_layer_bytes(int log2_layer_blocks) { return ((size_t)kDistBlockBytes << log2_layer_blocks) + kDistCounters * sizeof(u64); }

TsdfLayer tsdf_dist_layer(uint8_t* base, int log2_layer_blocks) {
    const size_t n = (size_t)1 << log2_layer_blocks;
    TsdfLayer L;
    uint8_t* p = base; // every part a multiple of 8 bytes but the last
    L.counters = reinterpret_cast<u64*>(p); p += kDistCounters * sizeof(u64);
    L.keys = reinterpret_cast<u64*>(p); p += n * 8;
    L.masks = reinterpret_cast<u64*>(p); p += n * kDistMaskWords * 8;
    L.cells = reinterpret_cast<uint16_t*>(p); p += n * kTsdfLanes * 2;
    L.tmp = reinterpret_cast<uint16_t*>(p); p += n * kTsdfLanes * 2;
    L.list = reinterpret_cast<uint32_t*>(p); p += n * 4;
    L.site_list = reinterpret_cast<uint32_t*>(p); p += n * 4;
    L.kind = p;
    L.log2_blocks = log2_layer_blocks;
    return L;
}

static unsigned dist_grid(size_t need) { return (unsigned)(need < 1 ? 1 : need > (size_t)kTsdfGrid ? (size_t)kTsdfGrid : need); }

int launch_tsdf_distance(const TsdfTable& t, const TsdfLayer& L, int map_id, int min_weight, int R, int form, unsigned long long* d_counts, hipStream_t stream) {
    const int rb = (R + 7) / 8;
    const size_t n_slots = (size_t)1 << L.log2_blocks;
    const unsigned g_layer = dist_grid(n_slots);
    {
        ProfScope ps(stream, "tsdf_dist_clear_kernel");
        hipLaunchKernelGGL(tsdf_dist_clear_kernel, dim3(dist_grid((n_slots * kDistMaskWords + kVoxelBlock - 1) / kVoxelBlock)), dim3(kVoxelBlock), 0, stream, L);
        VS_HIP(hipGetLastError());
    }
    {
        ProfScope ps(stream, "tsdf_dist_classify_kernel");
        hipLaunchKernelGGL(tsdf_dist_classify_kernel, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, L, map_id, (uint32_t)(min_weight < 1 ? 1 : min_weight));
        VS_HIP(hipGetLastError());
    }
    {
        ProfScope ps(stream, "tsdf_dist_dilate_kernel");
        hipLaunchKernelGGL(tsdf_dist_dilate_kernel, dim3(g_layer), dim3(kVoxelBlock), 0, stream, L, t.counters + 4, rb);
        VS_HIP(hipGetLastError());
    }
    if (form == 0) {
        ProfScope ps(stream, "tsdf_dist_brute_kernel");
        hipLaunchKernelGGL(tsdf_dist_brute_kernel, dim3(g_layer), dim3(kTsdfLanes), 0, stream, L, R, rb);
        VS_HIP(hipGetLastError());
    } else {
        {
            ProfScope ps(stream, "tsdf_dist_row_kernel");
            hipLaunchKernelGGL(tsdf_dist_row_kernel, dim3(g_layer), dim3(kTsdfLanes), 0, stream, L, R, rb);
            VS_HIP(hipGetLastError());
        }
        ProfScope ps(stream, "tsdf_dist_pass_kernel");
        hipLaunchKernelGGL(tsdf_dist_pass_kernel<1>, dim3(g_layer), dim3(kTsdfLanes), 0, stream, L, R, rb);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(tsdf_dist_pass_kernel<2>, dim3(g_layer), dim3(kTsdfLanes), 0, stream, L, R, rb);
        VS_HIP(hipGetLastError());
    }
    if (d_counts) {
        ProfScope ps(stream, "tsdf_dist_counts_kernel");
        hipLaunchKernelGGL(tsdf_dist_counts_kernel, dim3(1), dim3(64), 0, stream, L, d_counts);
        VS_HIP(hipGetLastError());
    }
    return VSLAM_OK;
}

int launch_tsdf_distance_blocks(const TsdfLayer& L, int map_id, int32_t* d_block_out, uint16_t* d_cells_out, size_t capacity, unsigned long long* d_n_out,
                                hipStream_t stream) {
    VS_HIP(hipMemsetAsync(d_n_out, 0, sizeof(u64), stream));
    ProfScope ps(stream, "tsdf_dist_blocks_kernel");
    hipLaunchKernelGGL(tsdf_dist_blocks_kernel, dim3(dist_grid((size_t)1 << L.log2_blocks)), dim3(kTsdfLanes), 0, stream, L, map_id, d_block_out, d_cells_out, (u64)capacity,
                       d_n_out);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_tsdf_distance_query(const TsdfTable& t, const TsdfLayer& L, const double* d_xyz_w, const int32_t* d_map_id, size_t N, float* d_dist, uint8_t* d_class,
                               hipStream_t stream) {
    ProfScope ps(stream, "tsdf_dist_query_kernel");
    constexpr size_t kMaxPoints = (size_t)1 << 30; // lanes a launch
    for (size_t n0 = 0; n0 < N; n0 += kMaxPoints) {
        const size_t n = N - n0 < kMaxPoints ? N - n0 : kMaxPoints;
        hipLaunchKernelGGL(tsdf_dist_query_kernel, dim3((unsigned)((n + kVoxelBlock - 1) / kVoxelBlock)), dim3(kVoxelBlock), 0, stream, L, (double)t.vs, d_xyz_w + 3 * n0,
                           d_map_id + n0, (u64)n, d_dist + n0, d_class + n0);
        VS_HIP(hipGetLastError());
    }
    return VSLAM_OK;
}

} // namespace vslam
