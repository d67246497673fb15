// PV-RCNN++'s VectorPool aggregation (pcd_ops.h section f6): the two-step three-NN of vector_pool_gpu.cu:19-205 as ONE kernel
// whose neighbour list lives in LDS, the interpolation + relative coordinates + empty-cell zeroing of
// pointnet2_modules.py:220-238 as one pass with its backward, and the voxel query of vector_pool_gpu.cu:243-458
// (pooling_type 1) with the winning row kept per cell instead of an atomically ordered list.  No atomics in any forward, no
// read-back, no buffer whose size depends on the data.
#include "common.h"

namespace {

constexpr int NN_CAP = PCD_VECTOR_POOL_MAX_NEIGHBORS;     // entries of a query's list (the reference's temp_idxs[1000])
constexpr int NN_QPB = PCD_VECTOR_POOL_NN_QUERIES_PER_WG; // one wave per query
constexpr int VQ_QPB = PCD_VECTOR_POOL_VQ_QUERIES_PER_WG; // one wave per query
constexpr int VQ_CHUNK = 1024;                            // support rows staged per step
constexpr int VQ_MAX_G = PCD_VECTOR_POOL_MAX_GRIDS;
static_assert(VQ_MAX_G == 64, "one bit per cell in a 64-bit mask, one LDS slot per lane");

// frame of query m (the reference's walk over new_xyz_batch_cnt: a query beyond the last count belongs to the last frame) and
// that frame's rows [start, start + n) of the support set, clipped to [0, N)
__device__ __forceinline__ void frame_of_query(int m, int B, int N, const int32_t *__restrict__ new_cnt,
                                               const int32_t *__restrict__ cnt, int &frame, int &start, int &n) {
    int b = 0, upto = new_cnt[0];
    for (int k = 1; k < B; ++k) {
        if (m < upto) break;
        upto += new_cnt[k];
        b = k;
    }
    long long s = 0;
    for (int k = 0; k < b; ++k) s += cnt[k] > 0 ? cnt[k] : 0;
    int c = cnt[b] > 0 ? cnt[b] : 0;
    if (s > N) s = N;
    if (c > N - (int)s) c = N - (int)s;
    frame = b, start = (int)s, n = c;
}

// cube / ball test of local = support - new, as vector_pool_gpu.cu:170-183 writes it
__device__ __forceinline__ bool outside(float lx, float ly, float lz, float r, float r2, int ball) {
    if (ball) return lx * lx + ly * ly + lz * lz > r2;
    return fabsf(lx) > r || fabsf(ly) > r || fabsf(lz) > r;
}

struct Top3 {
    float d0, d1, d2;
    int p0, p1, p2;                                        // list positions, -1: none
};

// (d, position) below slot k?  An empty slot loses to everything.
__device__ __forceinline__ bool before(float d, int p, float dk, int pk) { return pk < 0 || d < dk || (d == dk && p < pk); }

__device__ __forceinline__ void top3_insert(Top3 &t, float d, int p) {
    if (p < 0) return;
    if (before(d, p, t.d0, t.p0)) {
        t.d2 = t.d1, t.p2 = t.p1, t.d1 = t.d0, t.p1 = t.p0, t.d0 = d, t.p0 = p;
    } else if (before(d, p, t.d1, t.p1)) {
        t.d2 = t.d1, t.p2 = t.p1, t.d1 = d, t.p1 = p;
    } else if (before(d, p, t.d2, t.p2)) {
        t.d2 = d, t.p2 = p;
    }
}

// One wave per query.  Scan: the lanes test 64 consecutive rows of the query's frame per step (coalesced), ballot + prefix
// popcount append the hits to the wave's LDS list in ascending row order, and the scan ends at the cap.  Selection: lane =
// (part, centre); a part walks every P-th list entry for its centre, the parts meet through xor shuffles ordered by
// (d, position) -- the order the reference's sequential strict `<` produces.
__global__ __launch_bounds__(NN_QPB * 64) void vp_three_nn_kernel(int B, int M, int N, int G, float r, int cap, int ball,
                                                                  const float *__restrict__ sxyz, const int32_t *__restrict__ cnt,
                                                                  const float *__restrict__ new_xyz,
                                                                  const float *__restrict__ centers,
                                                                  const int32_t *__restrict__ new_cnt, int32_t *__restrict__ idx,
                                                                  float *__restrict__ dist2, int32_t *__restrict__ ncnt) {
    __shared__ float4 list[NN_QPB][NN_CAP];                // x, y, z, global row (as bits)
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int m = blockIdx.x * NN_QPB + w;
    const bool live = m < M;
    float4 *mine = list[w];
    int found = 0;
    if (live) {
        int frame, start, n;
        frame_of_query(m, B, N, new_cnt, cnt, frame, start, n);
        const float nx = new_xyz[(size_t)m * 3], ny = new_xyz[(size_t)m * 3 + 1], nz = new_xyz[(size_t)m * 3 + 2];
        const float r2 = r * r;
        for (int base = 0; base < n; base += 64) {
            const int k = base + lane;
            bool hit = false;
            float x = 0.f, y = 0.f, z = 0.f;
            if (k < n) {
                const float *p = sxyz + (size_t)(start + k) * 3;
                x = p[0], y = p[1], z = p[2];
                hit = !outside(x - nx, y - ny, z - nz, r, r2, ball);
            }
            int total;
            const int slot = found + wave_rank(hit, total);
            if (hit && slot < cap) mine[slot] = make_float4(x, y, z, __int_as_float(start + k));
            found += total;
            if (found >= cap) {
                found = cap;
                break;
            }
        }
    }
    __syncthreads();                                       // the list is written; every thread of the workgroup arrives here
    if (!live) return;
    if (lane == 0) ncnt[m] = found;
    int gp = 1;
    while (gp < G && gp < 64) gp <<= 1;                    // centres side by side in the wave
    const int parts = 64 / gp, part = lane / gp;
    for (int g0 = 0; g0 < G; g0 += gp) {
        const int g = g0 + (lane & (gp - 1));
        const bool has = g < G;
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (has) {
            const float *c = centers + ((size_t)m * G + g) * 3;
            cx = c[0], cy = c[1], cz = c[2];
        }
        Top3 t = {0.f, 0.f, 0.f, -1, -1, -1};
        for (int p = part; p < found; p += parts) {
            const float4 e = mine[p];
            const float d = (cx - e.x) * (cx - e.x) + (cy - e.y) * (cy - e.y) + (cz - e.z) * (cz - e.z);
            top3_insert(t, d, p);
        }
        for (int step = gp; step < 64; step <<= 1) {
            const float e0 = __shfl_xor(t.d0, step, 64), e1 = __shfl_xor(t.d1, step, 64), e2 = __shfl_xor(t.d2, step, 64);
            const int q0 = __shfl_xor(t.p0, step, 64), q1 = __shfl_xor(t.p1, step, 64), q2 = __shfl_xor(t.p2, step, 64);
            top3_insert(t, e0, q0), top3_insert(t, e1, q1), top3_insert(t, e2, q2);
        }
        if (has && part == 0) {
            int32_t *io = idx + ((size_t)m * G + g) * 3;
            float *dout = dist2 + ((size_t)m * G + g) * 3;
            if (t.p0 < 0) {
                io[0] = io[1] = io[2] = -1;
                dout[0] = dout[1] = dout[2] = __int_as_float(0x7f800000);       // the reference's 1e40 stored as float
            } else {
                if (t.p1 < 0) t.p1 = t.p0, t.d1 = t.d0;
                if (t.p2 < 0) t.p2 = t.p0, t.d2 = t.d0;
                io[0] = __float_as_int(mine[t.p0].w), io[1] = __float_as_int(mine[t.p1].w), io[2] = __float_as_int(mine[t.p2].w);
                dout[0] = t.d0, dout[1] = t.d1, dout[2] = t.d2;
            }
        }
    }
}

// the three weights of a cell (pointnet2_modules.py:220-222); false: an empty cell (or rows outside the support set)
__device__ __forceinline__ bool cell_weights(const int32_t *__restrict__ i3, const float *__restrict__ d3, int N, int row[3],
                                             float wgt[3]) {
    row[0] = i3[0], row[1] = i3[1], row[2] = i3[2];
    if ((unsigned)row[0] >= (unsigned)N || (unsigned)row[1] >= (unsigned)N || (unsigned)row[2] >= (unsigned)N) return false;
    const float r0 = 1.0f / (sqrtf(d3[0]) + 1e-8f), r1 = 1.0f / (sqrtf(d3[1]) + 1e-8f), r2 = 1.0f / (sqrtf(d3[2]) + 1e-8f);
    const float norm = fmaxf((r0 + r1) + r2, 1e-8f);
    wgt[0] = r0 / norm, wgt[1] = r1 / norm, wgt[2] = r2 / norm;
    return true;
}

// one thread per output element, consecutive threads along the C + 9 values of a cell: the store is one contiguous stream,
// the gathered feature rows are read in runs of C
__global__ __launch_bounds__(256) void vp_interp_fwd_kernel(long long total, int N, int C, const int32_t *__restrict__ idx,
                                                            const float *__restrict__ dist2, const float *__restrict__ sxyz,
                                                            const float *__restrict__ feat, const float *__restrict__ centers,
                                                            float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int width = C + 9;
    const long long cell = e / width;
    const int j = (int)(e - cell * width);
    int row[3];
    float wgt[3];
    float v = 0.f;
    if (cell_weights(idx + cell * 3, dist2 + cell * 3, N, row, wgt)) {
        if (j < C) {
            v = (wgt[0] * feat[(size_t)row[0] * C + j] + wgt[1] * feat[(size_t)row[1] * C + j]) + wgt[2] * feat[(size_t)row[2] * C + j];
        } else {
            const int s = (j - C) / 3, a = (j - C) - s * 3;
            v = centers[cell * 3 + a] - sxyz[(size_t)row[s] * 3 + a];
        }
    }
    out[e] = v;
}

// one thread per (cell, channel), consecutive threads along the channels: the atomics of a wave go to 3 * ceil(64 / C) rows
__global__ __launch_bounds__(256) void vp_interp_bwd_kernel(long long total, int N, int C, const int32_t *__restrict__ idx,
                                                            const float *__restrict__ dist2, const float *__restrict__ g,
                                                            float *__restrict__ d_feat) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long cell = e / C;
    const int c = (int)(e - cell * C);
    int row[3];
    float wgt[3];
    if (!cell_weights(idx + cell * 3, dist2 + cell * 3, N, row, wgt)) return;
    const float gv = g[cell * (C + 9) + c];
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(d_feat + (size_t)row[k] * C + c, wgt[k] * gv);
}

// One wave per query, VQ_QPB queries per workgroup.  The workgroup walks the frames its queries belong to (one, unless it
// straddles a frame border) and stages VQ_CHUNK support rows at a time in LDS; a wave tests 64 staged rows per step.  Of the
// hits of a step the lowest lane whose cell is still free takes it, then the next, ... : row order, as the reference's loop.
__global__ __launch_bounds__(VQ_QPB * 64) void vp_voxel_query_kernel(int B, int M, int N, int C, int ngx, int ngy, int ngz,
                                                                     float R, int want, int ball,
                                                                     const float *__restrict__ sxyz, const int32_t *__restrict__ cnt,
                                                                     const float *__restrict__ feat, const float *__restrict__ new_xyz,
                                                                     const int32_t *__restrict__ new_cnt, float *__restrict__ out,
                                                                     float *__restrict__ out_xyz, int32_t *__restrict__ out_cnt,
                                                                     int32_t *__restrict__ src_row) {
    __shared__ float stage[VQ_CHUNK * 3];
    __shared__ int32_t won[VQ_QPB][VQ_MAX_G];
    __shared__ float won_xyz[VQ_QPB][VQ_MAX_G * 3];
    const int w = threadIdx.x >> 6, lane = lane_id(), G = ngx * ngy * ngz;
    const int m_first = blockIdx.x * VQ_QPB, m = m_first + w;
    const bool live = m < M;
    const int m_last = min(M, m_first + VQ_QPB) - 1;
    int f_first, f_last, my_frame = -1, start, n;
    frame_of_query(m_first, B, N, new_cnt, cnt, f_first, start, n);
    frame_of_query(m_last, B, N, new_cnt, cnt, f_last, start, n);
    if (live) frame_of_query(m, B, N, new_cnt, cnt, my_frame, start, n);
    won[w][lane] = -1;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (live) nx = new_xyz[(size_t)m * 3], ny = new_xyz[(size_t)m * 3 + 1], nz = new_xyz[(size_t)m * 3 + 2];
    const float r2 = R * R;
    const float gsx = R * 2 / ngx, gsy = R * 2 / ngy, gsz = R * 2 / ngz;
    u64 filled = 0;
    int nfilled = 0;
    bool done = !live;
    for (int f = f_first; f <= f_last; ++f) {
        int fs, fn;
        {                                                  // rows of frame f, as frame_of_query clips them
            long long s = 0;
            for (int k = 0; k < f; ++k) s += cnt[k] > 0 ? cnt[k] : 0;
            int c = cnt[f] > 0 ? cnt[f] : 0;
            if (s > N) s = N;
            if (c > N - (int)s) c = N - (int)s;
            fs = (int)s, fn = c;
        }
        for (int c0 = 0; c0 < fn; c0 += VQ_CHUNK) {
            const int rows = min(VQ_CHUNK, fn - c0);
            __syncthreads();                               // the previous chunk has been read
            for (int i = threadIdx.x; i < rows * 3; i += VQ_QPB * 64) stage[i] = sxyz[(size_t)(fs + c0) * 3 + i];
            __syncthreads();
            const bool mine = !done && my_frame == f;
            if (mine) {
                for (int base = 0; base < rows; base += 64) {
                    const int k = base + lane;
                    bool cand = false;
                    int cell = 0;
                    float lx = 0.f, ly = 0.f, lz = 0.f;
                    if (k < rows) {
                        lx = stage[k * 3] - nx, ly = stage[k * 3 + 1] - ny, lz = stage[k * 3 + 2] - nz;
                        if (!outside(lx, ly, lz, R, r2, ball)) {
                            const int ix = (int)floorf((lx + R) / gsx), iy = (int)floorf((ly + R) / gsy), iz = (int)floorf((lz + R) / gsz);
                            cell = ix * ngy * ngz + iy * ngz + iz;
                            cell = min(max(cell, 0), G - 1);
                            cand = !((filled >> cell) & 1ull);
                        }
                    }
                    u64 pending = __ballot(cand);
                    while (pending) {
                        const int first = __ffsll((long long)pending) - 1;
                        const int its_cell = __shfl(cell, first, 64);
                        if (lane == first) {
                            won[w][cell] = fs + c0 + k;
                            won_xyz[w][cell * 3] = lx, won_xyz[w][cell * 3 + 1] = ly, won_xyz[w][cell * 3 + 2] = lz;
                        }
                        filled |= 1ull << its_cell;
                        if (++nfilled >= want) {
                            done = true;
                            break;
                        }
                        if (cand && cell == its_cell) cand = false;
                        pending = __ballot(cand);
                    }
                    if (done) break;
                }
            }
            if (!__syncthreads_or(!done && my_frame == f)) break;      // no query of this frame needs another chunk
        }
    }
    __syncthreads();
    if (!live) return;
    if (lane < G) {
        const int row = won[w][lane];
        const bool has = (unsigned)row < (unsigned)N;
        src_row[(size_t)m * G + lane] = has ? row : -1;
        out_cnt[(size_t)m * G + lane] = has ? 1 : 0;
    }
    for (int i = lane; i < G * 3; i += 64) out_xyz[(size_t)m * G * 3 + i] = (unsigned)won[w][i / 3] < (unsigned)N ? won_xyz[w][i] : 0.f;
    for (int i = lane; i < G * C; i += 64) {
        const int g = i / C, c = i - g * C, row = won[w][g];
        out[(size_t)m * G * C + i] = (unsigned)row < (unsigned)N ? feat[(size_t)row * C + c] : 0.f;
    }
}

// one thread per (query, cell, channel), consecutive threads along the channels
__global__ __launch_bounds__(256) void vp_voxel_query_bwd_kernel(long long total, int N, int C, const float *__restrict__ g,
                                                                 const int32_t *__restrict__ src_row, float *__restrict__ d_feat) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long cell = e / C;
    const int c = (int)(e - cell * C), row = src_row[cell];
    if ((unsigned)row < (unsigned)N) atomicAdd(d_feat + (size_t)row * C + c, g[e]);
}

inline bool grid_fits(long long elements, int per_block) { return (elements + per_block - 1) / per_block <= 0x7fffffffLL; }

}  // namespace

extern "C" int pcd_vector_pool_three_nn(int B, int M, int N, int G, const float *support_xyz, const int32_t *xyz_batch_cnt,
                                        const float *new_xyz, const float *new_xyz_grid_centers,
                                        const int32_t *new_xyz_batch_cnt, float query_distance, int nsample, int neighbor_type,
                                        int32_t *idx, float *dist2, int32_t *neighbor_cnt, void *stream) {
    PCD_ENTER();
    if (B <= 0 || M < 0 || N < 0 || G <= 0) return PCD_ERR_INVALID_ARG;
    if (M == 0 || N == 0) return PCD_OK;                   // (no support rows: the caller's buffers hold the empty result)
    if (!new_xyz || !new_xyz_grid_centers || !new_xyz_batch_cnt || !xyz_batch_cnt || !idx || !dist2 || !neighbor_cnt || !support_xyz)
        return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int cap = nsample > 0 && nsample < NN_CAP ? nsample : NN_CAP;
    vp_three_nn_kernel<<<pcd_div_up(M, NN_QPB), NN_QPB * 64, 0, st>>>(B, M, N, G, query_distance, cap, neighbor_type == 1,
                                                                     support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers,
                                                                     new_xyz_batch_cnt, idx, dist2, neighbor_cnt);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_vector_pool_interpolate_forward(int M, int N, int G, int C, const int32_t *idx, const float *dist2,
                                                   const float *support_xyz, const float *support_features,
                                                   const float *new_xyz_grid_centers, float *out, void *stream) {
    PCD_ENTER();
    if (M < 0 || N < 0 || G <= 0 || C <= 0) return PCD_ERR_INVALID_ARG;
    if (M == 0 || N == 0) return PCD_OK;                   // (no support rows: the caller's buffer holds the zeros)
    if (!idx || !dist2 || !new_xyz_grid_centers || !out || !support_xyz || !support_features) return PCD_ERR_INVALID_ARG;
    const long long total = (long long)M * G * (C + 9);
    if (!grid_fits(total, 256)) return PCD_ERR_UNSUPPORTED;
    vp_interp_fwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(total, N, C, idx, dist2, support_xyz,
                                                                                           support_features,
                                                                                           new_xyz_grid_centers, out);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_vector_pool_interpolate_backward(int M, int N, int G, int C, const int32_t *idx, const float *dist2,
                                                    const float *grad_out, float *grad_support_features_zeroed, void *stream) {
    PCD_ENTER();
    if (M < 0 || N < 0 || G <= 0 || C <= 0) return PCD_ERR_INVALID_ARG;
    if (M == 0 || N == 0) return PCD_OK;
    if (!idx || !dist2 || !grad_out || !grad_support_features_zeroed) return PCD_ERR_INVALID_ARG;
    const long long total = (long long)M * G * C;
    if (!grid_fits(total, 256)) return PCD_ERR_UNSUPPORTED;
    vp_interp_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(total, N, C, idx, dist2, grad_out,
                                                                                           grad_support_features_zeroed);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_vector_pool_voxel_query_forward(int B, int M, int N, int num_c_in, int num_c_out_each_grid, int num_grid_x,
                                                   int num_grid_y, int num_grid_z, float max_neighbour_distance, int nsample,
                                                   int neighbor_type, int pooling_type, const float *support_xyz,
                                                   const int32_t *xyz_batch_cnt, const float *support_features,
                                                   const float *new_xyz, const int32_t *new_xyz_batch_cnt, float *new_features,
                                                   float *new_local_xyz, int32_t *point_cnt_of_grid, int32_t *src_row,
                                                   void *stream) {
    PCD_ENTER();
    if (B <= 0 || M < 0 || N < 0 || num_c_in <= 0 || num_grid_x <= 0 || num_grid_y <= 0 || num_grid_z <= 0)
        return PCD_ERR_INVALID_ARG;
    if (pooling_type != 1) return PCD_ERR_INVALID_ARG;     // voxel_avg_pool: no configuration of the reference uses it
    if (num_c_in != num_c_out_each_grid) return PCD_ERR_INVALID_ARG;   // (the reference's forward and backward disagree there)
    const long long G = (long long)num_grid_x * num_grid_y * num_grid_z;
    if (G > VQ_MAX_G) return PCD_ERR_UNSUPPORTED;
    if (M == 0 || N == 0) return PCD_OK;                   // (no support rows: the caller's buffers hold the empty result)
    if (!new_xyz || !new_xyz_batch_cnt || !xyz_batch_cnt || !new_features || !new_local_xyz || !point_cnt_of_grid || !src_row ||
        !support_xyz || !support_features)
        return PCD_ERR_INVALID_ARG;
    const int want = nsample > 0 && nsample < (int)G ? nsample : (int)G;
    vp_voxel_query_kernel<<<pcd_div_up(M, VQ_QPB), VQ_QPB * 64, 0, (hipStream_t)stream>>>(
        B, M, N, num_c_in, num_grid_x, num_grid_y, num_grid_z, max_neighbour_distance, want, neighbor_type == 1, support_xyz,
        xyz_batch_cnt, support_features, new_xyz, new_xyz_batch_cnt, new_features, new_local_xyz, point_cnt_of_grid, src_row);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_vector_pool_voxel_query_backward(int M, int N, int G, int C, const float *grad_new_features,
                                                    const int32_t *src_row, float *grad_support_features_zeroed, void *stream) {
    PCD_ENTER();
    if (M < 0 || N < 0 || G <= 0 || C <= 0) return PCD_ERR_INVALID_ARG;
    if (M == 0 || N == 0) return PCD_OK;
    if (!grad_new_features || !src_row || !grad_support_features_zeroed) return PCD_ERR_INVALID_ARG;
    const long long total = (long long)M * G * C;
    if (!grid_fits(total, 256)) return PCD_ERR_UNSUPPORTED;
    vp_voxel_query_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(total, N, C, grad_new_features,
                                                                                                src_row,
                                                                                                grad_support_features_zeroed);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
