// tsdf_mesh_kernels.hip -- the surface map's triangle mesh (include/vslam_hip.h "MESH") and the block loader.
//
//   tsdf_mesh_vertex_kernel   tsdf_extract_kernel's walk: block in LDS, one lane per voxel, its three edges; a crossing edge takes the next vertex index
//                             (one counter add per wave and axis), leaves as EXTRACTION's surfel while the index is below the capacity, and the index
//                             goes into the vertex-id table vid[list position][axis][voxel] (-1: nothing crosses); pos_of_slot[slot] = list position
//   tsdf_mesh_tri_kernel      one lane per cell (the cell whose lowest corner is the lane's voxel): the good and sign bits of the block and of the
//                             +1 faces, edges and corner of up to seven neighbour blocks staged as 9 x 9 x 9 bytes in LDS (one table lookup per
//                             neighbour block and workgroup), the cell's row of k_mc_table, a wave prefix sum of the rows' triangle counts (one counter
//                             add per wave), every corner's index read from vid of the block that owns the edge's lower voxel
//   tsdf_load_kernel          one workgroup per listed block: lane 0 claims it, 512 lanes copy its voxels
// Connectivity is an integer function of the field (the sign rule and good() are exact), so the mesh is held to tests/tsdf_mesh_ref.py exactly.
// No lane waits on another, no floating-point atomics, every store is guarded by its capacity and every list position read from the tables is
// range-checked before it indexes vid.  Compiled with FMA contraction off: the vertices are the extraction's bits.
#include "vslam_internal.h"

#include "tsdf_device.h"

namespace vslam {

#include "mc_table.inc"

// the vertex-id table of a mesh call: vid holds 3 x 512 int32 per list position below n_pos, pos_of_slot one uint32 per slot of the pool
struct TsdfMeshTable { int32_t* vid; uint32_t* pos_of_slot; u64 n_pos; };

__global__ __launch_bounds__(kTsdfLanes) void tsdf_mesh_vertex_kernel(TsdfTable t, TsdfMeshTable mt, int map_id, uint32_t min_w, vslam_surfel* __restrict__ out,
                                                                      int32_t* __restrict__ map_out, u64 capacity, u64* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ uint4 lv[kTsdfLanes];
    const u64 n_list = t.counters[0] < mt.n_pos ? t.counters[0] : mt.n_pos;
    const int l = threadIdx.x, lane = l & 63;
    const double vs = (double)t.vs;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = t.list[i];
        if (l == 0) mt.pos_of_slot[s] = (uint32_t)i; // (s < 2^log2_blocks: only claimed slots enter the list)
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        if (map_id >= 0 && id.map != map_id) continue; // (workgroup-uniform)
        __syncthreads(); // (the readers of the last block are done)
        const uint4 va = t.pool[(size_t)s * kTsdfLanes + l];
        lv[l] = va;
        __syncthreads();
        if (va.x >= kTsdfMaxW) atomicOr(&t.counters[4], 2ull);
        const int ia[3] = {id.bx * 8 + (l & 7), id.by * 8 + ((l >> 3) & 7), id.bz * 8 + (l >> 6)};
        const bool good_a = tsdf_good(va, min_w);
        const double Da = good_a ? tsdf_D(va) : 0.0;
#pragma unroll 1
        for (int e = 0; e < 3; ++e) {
            const int e0 = e == 0, e1 = e == 1, e2 = e == 2;
            bool take = false;
            uint4 vb = make_uint4(0u, 0u, 0u, 0u);
            if (good_a) {
                vb = tsdf_fetch(t, lv, id, ia[0] + e0, ia[1] + e1, ia[2] + e2);
                take = tsdf_good(vb, min_w) && ((tsdf_num(va) > 0) != (tsdf_num(vb) > 0));
            }
            const u64 ballot = __ballot(take);
            u64 first = 0;
            if (ballot != 0 && lane == 0) first = atomicAdd(&counts[0], (u64)__popcll(ballot));
            first = __shfl(first, 0);
            const u64 pos = first + (u64)__popcll(ballot & ((1ull << lane) - 1ull));
            // (every entry of a walked block is written; an index past int32 cannot be a triangle corner)
            mt.vid[(i * 3 + (u64)e) * kTsdfLanes + l] = (take && pos <= 0x7FFFFFFFull) ? (int32_t)pos : -1;
            if (!take || pos >= capacity) continue;
            tsdf_surfel(t, lv, id, ia, e, va, vb, Da, min_w, vs, out + pos);
            if (map_out) map_out[pos] = id.map;
        }
    }
}

// the good bit (1) and the sign bit (2: num > 0) of a voxel
__device__ __forceinline__ uint32_t tsdf_mesh_bits(const uint4& v, uint32_t min_w) { return (tsdf_good(v, min_w) ? 1u : 0u) | (tsdf_num(v) > 0 ? 2u : 0u); }

__global__ __launch_bounds__(kTsdfLanes) void tsdf_mesh_tri_kernel(TsdfTable t, TsdfMeshTable mt, int map_id, uint32_t min_w, vslam_triangle* __restrict__ tri_out,
                                                                   u64 capacity, u64* __restrict__ counts) {
    __shared__ uint8_t bits[9 * 9 * 9];
    __shared__ int32_t nb_slot[8];  // slot of the neighbour block (dx | dy << 1 | dz << 2), -1: not claimed or outside the index range
    __shared__ int32_t nb_pos[8];   // ... and its list position, -1: none that vid holds
    const u64 n_list = t.counters[0] < mt.n_pos ? t.counters[0] : mt.n_pos;
    const uint32_t n_slots = 1u << t.log2_blocks;
    const int l = threadIdx.x, lane = l & 63;
    const int x = l & 7, y = (l >> 3) & 7, z = l >> 6;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = t.list[i];
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        if (map_id >= 0 && id.map != map_id) continue; // (workgroup-uniform)
        __syncthreads(); // (the readers of the last block are done)
        if (l < 8) {
            const int bx = id.bx + (l & 1), by = id.by + ((l >> 1) & 1), bz = id.bz + (l >> 2);
            int32_t slot = -1, pos = -1;
            if (l == 0) { slot = (int32_t)s; pos = (int32_t)i; }
            else if (bx < kTsdfBHalf && by < kTsdfBHalf && bz < kTsdfBHalf) {
                uint32_t f;
                const u64 key = (u64)(uint32_t)id.map << 45 | (u64)(uint32_t)(bx + kTsdfBHalf) << 30 | (u64)(uint32_t)(by + kTsdfBHalf) << 15 | (u64)(uint32_t)(bz + kTsdfBHalf);
                if (tsdf_find(t, key, f) && f < n_slots) {
                    slot = (int32_t)f;
                    const uint32_t p = mt.pos_of_slot[f];
                    if ((u64)p < n_list && t.list[p] == f) pos = (int32_t)p; // (the vertex pass of this call wrote it; anything else is not trusted)
                }
            }
            nb_slot[l] = slot; nb_pos[l] = pos;
        }
        __syncthreads();
        for (int c = l; c < 9 * 9 * 9; c += kTsdfLanes) {
            const int cx = c % 9, cy = (c / 9) % 9, cz = c / 81;
            const int32_t slot = nb_slot[(cx >> 3) | (cy >> 3) << 1 | (cz >> 3) << 2];
            uint32_t b = 0u;
            if (slot >= 0) b = tsdf_mesh_bits(t.pool[(size_t)slot * kTsdfLanes + ((cz & 7) << 6 | (cy & 7) << 3 | (cx & 7))], min_w);
            bits[c] = (uint8_t)b;
        }
        __syncthreads();
        uint32_t all_good = 1u, cube = 0u;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t b = bits[((z + (c >> 2)) * 9 + y + ((c >> 1) & 1)) * 9 + x + (c & 1)];
            all_good &= b; cube |= (b >> 1) << c;
        }
        const u64 row = (all_good & 1u) ? k_mc_table[cube & 255u] : 0ull;
        const uint32_t n_tri = (uint32_t)(row >> 60);
        // the wave's prefix sum of n_tri (0 .. 5): three ballots, one per bit
        const u64 below = (1ull << lane) - 1ull;
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const u64 m = __ballot((n_tri >> b) & 1u);
            before += (uint32_t)__popcll(m & below) << b; total += (uint32_t)__popcll(m) << b;
        }
        if (total == 0u) continue; // (wave-uniform)
        u64 first = 0;
        if (lane == 0) first = atomicAdd(&counts[1], (u64)total);
        first = __shfl(first, 0) + before;
        for (uint32_t j = 0; j < n_tri; ++j) {
            if (first + j >= capacity) break;
            int32_t v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t k = (uint32_t)(row >> (12 * j + 4 * c)) & 15u, e = k >> 2, p = k & 1u, q = (k >> 1) & 1u;
                // the edge's lower voxel: the cell's corner p f^ + q g^, f = (e + 1) % 3, g = (e + 2) % 3
                const int vx = x + (int)(e == 2 ? p : e == 1 ? q : 0u), vy = y + (int)(e == 0 ? p : e == 2 ? q : 0u), vz = z + (int)(e == 1 ? p : e == 0 ? q : 0u);
                const int32_t pos = nb_pos[(vx >> 3) | (vy >> 3) << 1 | (vz >> 3) << 2];
                v[c] = (pos >= 0 && e < 3u) ? mt.vid[((u64)pos * 3 + e) * kTsdfLanes + ((vz & 7) << 6 | (vy & 7) << 3 | (vx & 7))] : -1;
            }
            int32_t* o = tri_out[first + j].v;
            o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
        }
    }
}

// d_ids: n x (map, bx, by, bz); d_voxels: n x 512 uint4.  A block whose id is out of range counts in counters[2]; one that finds no slot in
// counters[3] and sets status bit 0 (tsdf_claim's rule); nothing is written for either.
__global__ __launch_bounds__(kTsdfLanes) void tsdf_load_kernel(TsdfTable t, const int4* __restrict__ ids, const uint4* __restrict__ voxels, u64 n) {
    __shared__ int32_t s_slot;
    const uint32_t n_slots = 1u << t.log2_blocks;
    const int l = threadIdx.x;
    for (u64 i = blockIdx.x; i < n; i += gridDim.x) {
        __syncthreads(); // (the readers of the last slot are done)
        if (l == 0) {
            const int4 id = ids[i];
            int32_t slot = -1;
            const bool inr = id.x >= 0 && id.x <= kVoxelMaxMap && id.y >= -kTsdfBHalf && id.y < kTsdfBHalf && id.z >= -kTsdfBHalf && id.z < kTsdfBHalf &&
                             id.w >= -kTsdfBHalf && id.w < kTsdfBHalf;
            if (!inr) atomicAdd(&t.counters[2], 1ull);
            else {
                const u64 key = (u64)(uint32_t)id.x << 45 | (u64)(uint32_t)(id.y + kTsdfBHalf) << 30 | (u64)(uint32_t)(id.z + kTsdfBHalf) << 15 | (u64)(uint32_t)(id.w + kTsdfBHalf);
                TsdfTally tally;
                tsdf_claim(t, key, 1u, tally);
                uint32_t f;
                if (tally.full) { atomicAdd(&t.counters[3], 1ull); atomicOr(&t.counters[4], 1ull); }
                else if (tsdf_find(t, key, f) && f < n_slots) slot = (int32_t)f;
            }
            s_slot = slot;
        }
        __syncthreads();
        const int32_t slot = s_slot;
        if (slot < 0) continue; // (workgroup-uniform)
        t.pool[(size_t)slot * kTsdfLanes + l] = voxels[i * kTsdfLanes + l];
    }
}

// ------------------------------------------------------------------------------------------------------------------- launchers
// vid_blocks: the list positions `vid` holds (>= the claimed blocks at the time of the call)
int launch_tsdf_mesh(const TsdfTable& t, int32_t* d_vid, uint32_t* d_pos_of_slot, size_t vid_blocks, int map_id, int min_weight, vslam_surfel* d_vertices,
                     int32_t* d_vertex_map, size_t vertex_capacity, vslam_triangle* d_triangles, size_t triangle_capacity, unsigned long long* d_counts,
                     hipStream_t stream) {
    VS_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(u64), stream));
    const TsdfMeshTable mt{d_vid, d_pos_of_slot, (u64)vid_blocks};
    const uint32_t min_w = (uint32_t)(min_weight < 1 ? 1 : min_weight);
    {
        ProfScope ps(stream, "tsdf_mesh_vertex_kernel");
        hipLaunchKernelGGL(tsdf_mesh_vertex_kernel, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, mt, map_id, min_w, d_vertices, d_vertex_map, (u64)vertex_capacity,
                           d_counts);
        VS_HIP(hipGetLastError());
    }
    ProfScope ps(stream, "tsdf_mesh_tri_kernel");
    hipLaunchKernelGGL(tsdf_mesh_tri_kernel, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, mt, map_id, min_w, d_triangles, (u64)triangle_capacity, d_counts);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_tsdf_load(const TsdfTable& t, const int32_t* d_block_ids, const uint32_t* d_voxels, size_t n, hipStream_t stream) {
    if (n == 0) return VSLAM_OK;
    ProfScope ps(stream, "tsdf_load_kernel");
    hipLaunchKernelGGL(tsdf_load_kernel, dim3((unsigned)(n < (size_t)kTsdfGrid ? n : (size_t)kTsdfGrid)), dim3(kTsdfLanes), 0, stream, t,
                       reinterpret_cast<const int4*>(d_block_ids), reinterpret_cast<const uint4*>(d_voxels), (u64)n);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
