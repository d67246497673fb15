// Voxel R-CNN's RoI-grid pooling (pcd_ops.h section f5): the voxel -> row map of generate_voxel2pinds
// (pcdet/utils/common_utils.py:244-252), the cooperative voxel query (voxel_query_gpu.cu:10-88) with the moments BatchNorm2d
// needs of the relative coordinates, and the fused gather + position affine + ReLU + max-pool of NeighborVoxelSAModuleMSG
// (voxel_pool_modules.py:96-116) with its backward through the saved winner.  No [M][C][nsample] tensor exists.
#include "common.h"

namespace {

constexpr int VP_G = PCD_VOXEL_POOL_GROUP;                // lanes per query
constexpr int VP_QPB = 256 / VP_G;                        // queries per workgroup
constexpr int VP_BWD_QPB = PCD_VOXEL_POOL_BWD_QUERIES_PER_WG;
static_assert(VP_QPB == PCD_VOXEL_POOL_QUERIES_PER_WG && (VP_G & (VP_G - 1)) == 0 && VP_G <= 32, "group layout");

// scatter (value = row) / clear (value = -1) of the rows of a level into the dense map
__global__ __launch_bounds__(256) void v2p_kernel(const int32_t *__restrict__ indices, int n_cap,
                                                  const int32_t *__restrict__ num_rows, int32_t *__restrict__ map, int B, int Z,
                                                  int Y, int X, int clear) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= eff_rows(num_rows, n_cap)) return;
    const int32_t *c = indices + (size_t)i * 4;
    const int b = c[0], z = c[1], y = c[2], x = c[3];
    if ((unsigned)b >= (unsigned)B || (unsigned)z >= (unsigned)Z || (unsigned)y >= (unsigned)Y || (unsigned)x >= (unsigned)X) return;
    map[(((size_t)b * Z + z) * Y + y) * X + x] = clear ? -1 : i;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;                                              // (lane 0 holds the sum; a fixed tree)
}

// VP_G lanes per query probe VP_G consecutive cells of the (dz, dy, dx) scan order per step; the hits of a step keep their
// order through the group's bits of the ballot.  The lane that finds a hit holds its relative coordinates: the moments cost
// no second pass.
__global__ __launch_bounds__(256) void vp_query_kernel(int M, int N, int B, int R1, int R2, int R3, int nsample, float radius,
                                                       int zr, int yr, int xr, const float *__restrict__ new_xyz,
                                                       const float *__restrict__ xyz, const int32_t *__restrict__ new_coords,
                                                       const int32_t *__restrict__ map, int32_t *__restrict__ idx,
                                                       int32_t *__restrict__ cnt_out, double *__restrict__ partial) {
    __shared__ double red[4][9];
    const int gl = threadIdx.x & (VP_G - 1);
    const int q = blockIdx.x * VP_QPB + (threadIdx.x / VP_G);
    const int shift = lane_id() & ~(VP_G - 1);             // where this group's bits start in the wave's ballot
    const bool live = q < M;
    const int nxs = 2 * xr + 1, nys = 2 * yr + 1, T = nxs * nys * (2 * zr + 1);
    const float r2 = radius * radius;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    int cb = -1, cz = 0, cy = 0, cx = 0;
    if (live) {
        nx = new_xyz[(size_t)q * 3], ny = new_xyz[(size_t)q * 3 + 1], nz = new_xyz[(size_t)q * 3 + 2];
        const int32_t *cd = new_coords + (size_t)q * 4;
        cb = cd[0], cz = cd[1], cy = cd[2], cx = cd[3];
    }
    bool active = live && (unsigned)cb < (unsigned)B;
    int cnt = 0, first_nb = 0;
    bool has_first = false;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int base = 0; base < T; base += VP_G) {
        if (!__any(active)) break;
        const int t = base + gl;
        bool hit = false;
        int nb = -1;
        float rx = 0.f, ry = 0.f, rz = 0.f;
        if (active && t < T) {
            const int dz = t / (nys * nxs), rem = t - dz * (nys * nxs), dy = rem / nxs, dx = rem - dy * nxs;
            const int z = cz + dz - zr, y = cy + dy - yr, x = cx + dx - xr;
            if ((unsigned)z < (unsigned)R1 && (unsigned)y < (unsigned)R2 && (unsigned)x < (unsigned)R3) {
                nb = map[(((size_t)cb * R1 + z) * R2 + y) * R3 + x];
                if ((unsigned)nb < (unsigned)N) {
                    rx = xyz[(size_t)nb * 3] - nx, ry = xyz[(size_t)nb * 3 + 1] - ny, rz = xyz[(size_t)nb * 3 + 2] - nz;
                    hit = !(rx * rx + ry * ry + rz * rz > r2);
                }
            }
        }
        const u32 gm = (u32)(__ballot(hit) >> shift) & ((1u << VP_G) - 1u);
        const int slot = cnt + __popc(gm & ((1u << gl) - 1u));
        if (hit && slot < nsample) {
            idx[(size_t)q * nsample + slot] = nb;
            const double x = rx, y = ry, z = rz;
            acc[0] += x, acc[1] += y, acc[2] += z;
            acc[3] += x * x, acc[4] += x * y, acc[5] += x * z, acc[6] += y * y, acc[7] += y * z, acc[8] += z * z;
            if (slot == 0) has_first = true, first_nb = nb, fx = rx, fy = ry, fz = rz;
        }
        cnt += __popc(gm);
        if (cnt >= nsample) cnt = nsample, active = false;
    }
    // the slots behind the last hit repeat the first hit (an empty ball: all 0, and r = 0 in the moments)
    const u32 fm = (u32)(__ballot(has_first) >> shift) & ((1u << VP_G) - 1u);
    const int first = __shfl(first_nb, fm ? shift + __ffs(fm) - 1 : lane_id(), 64);
    if (live) {
        const int fill = fm ? first : 0;
        for (int s = cnt + gl; s < nsample; s += VP_G) idx[(size_t)q * nsample + s] = fill;
        if (gl == 0) cnt_out[q] = cnt;
    }
    if (has_first) {
        const double w = (double)(nsample - cnt), x = fx, y = fy, z = fz;
        acc[0] += w * x, acc[1] += w * y, acc[2] += w * z;
        acc[3] += w * (x * x), acc[4] += w * (x * y), acc[5] += w * (x * z), acc[6] += w * (y * y), acc[7] += w * (y * z),
            acc[8] += w * (z * z);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double s = wave_sum_f64(acc[k]);
        if (lane_id() == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 9)
        partial[(size_t)blockIdx.x * 9 + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// wave k joins moment k: lane l sums the partials l, l + 64, ... in order, then the fixed tree
__global__ __launch_bounds__(576) void vp_join_moments_kernel(const double *__restrict__ partial, int nwg,
                                                              double *__restrict__ moments) {
    const int k = threadIdx.x >> 6;
    double s = 0.0;
    for (int w = lane_id(); w < nwg; w += 64) s += partial[(size_t)w * 9 + k];
    s = wave_sum_f64(s);
    if (lane_id() == 0) moments[k] = s;
}

__device__ __forceinline__ float relu_f32(float v) { return v > 0.f ? v : 0.f; }

// W lanes along c per query (a gathered row of fin is one coalesced read), 256 / W queries per workgroup
template <int W>
__global__ __launch_bounds__(256) void vp_fwd_kernel(int M, int N, int C, int nsample, const float *__restrict__ fin,
                                                     const float *__restrict__ A, const float *__restrict__ bvec,
                                                     const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                     const int32_t *__restrict__ idx, const int32_t *__restrict__ cnt,
                                                     float *__restrict__ out, unsigned char *__restrict__ arg) {
    const int m = blockIdx.x * (256 / W) + threadIdx.x / W;
    if (m >= M) return;
    int n = cnt[m];
    n = n < nsample ? (n < 0 ? 0 : n) : nsample;
    const float nx = new_xyz[(size_t)m * 3], ny = new_xyz[(size_t)m * 3 + 1], nz = new_xyz[(size_t)m * 3 + 2];
    const int32_t *rows = idx + (size_t)m * nsample;
    for (int c = threadIdx.x % W; c < C; c += W) {
        const float a0 = A[c * 3], a1 = A[c * 3 + 1], a2 = A[c * 3 + 2], bb = bvec[c];
        float best = -1.f;                                 // below every relu value
        int win = 0;
#pragma unroll 4
        for (int s = 0; s < n; ++s) {
            const int row = rows[s];
            if ((unsigned)row >= (unsigned)N) continue;
            const float rx = xyz[(size_t)row * 3] - nx, ry = xyz[(size_t)row * 3 + 1] - ny, rz = xyz[(size_t)row * 3 + 2] - nz;
            const float v = relu_f32(fin[(size_t)row * C + c] + (((a0 * rx + a1 * ry) + a2 * rz) + bb));
            if (v > best) best = v, win = s;
        }
        if (best < 0.f) best = relu_f32(bb), win = 0;      // an empty ball: grouped features 0, r = 0
        out[(size_t)m * C + c] = best;
        arg[(size_t)m * C + c] = (unsigned char)win;
    }
}

// one workgroup takes VP_BWD_QPB queries, 256 / W at a time; every thread keeps (dA0, dA1, dA2, db) of its channels, the
// groups of a workgroup meet in LDS in a fixed order
template <int W>
__global__ __launch_bounds__(256) void vp_bwd_kernel(int M, int N, int C, int nsample, const float *__restrict__ g,
                                                     const float *__restrict__ out, const unsigned char *__restrict__ arg,
                                                     const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                     const int32_t *__restrict__ idx, const int32_t *__restrict__ cnt,
                                                     float *__restrict__ d_fin, float *__restrict__ partial) {
    constexpr int GROUPS = 256 / W, PASSES = PCD_VOXEL_POOL_MAX_C / W;
    extern __shared__ float lds[];                         // [GROUPS][C][4]
    const int grp = threadIdx.x / W, c0 = threadIdx.x % W;
    float acc[PASSES][4];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) acc[p][0] = acc[p][1] = acc[p][2] = acc[p][3] = 0.f;
    const int m_end = min(M, (int)(blockIdx.x + 1) * VP_BWD_QPB);
    for (int m = blockIdx.x * VP_BWD_QPB + grp; m < m_end; m += GROUPS) {
        const int n = cnt[m];
        const float nx = new_xyz[(size_t)m * 3], ny = new_xyz[(size_t)m * 3 + 1], nz = new_xyz[(size_t)m * 3 + 2];
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int c = c0 + p * W;
            if (c >= C) break;
            const size_t e = (size_t)m * C + c;
            if (!(out[e] > 0.f)) continue;
            const float gv = g[e];
            acc[p][3] += gv;
            if (n <= 0) continue;                          // an empty ball: r = 0, no feature gradient
            const int s = arg[e];
            const int row = s < nsample ? idx[(size_t)m * nsample + s] : -1;
            if ((unsigned)row >= (unsigned)N) continue;
            acc[p][0] += gv * (xyz[(size_t)row * 3] - nx);
            acc[p][1] += gv * (xyz[(size_t)row * 3 + 1] - ny);
            acc[p][2] += gv * (xyz[(size_t)row * 3 + 2] - nz);
            atomicAdd(d_fin + (size_t)row * C + c, gv);
        }
    }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int c = c0 + p * W;
        if (c < C) {
#pragma unroll
            for (int k = 0; k < 4; ++k) lds[((size_t)grp * C + c) * 4 + k] = acc[p][k];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < C * 4; e += 256) {
        float s = 0.f;
        for (int gi = 0; gi < GROUPS; ++gi) s += lds[(size_t)gi * C * 4 + e];
        partial[(size_t)blockIdx.x * C * 4 + e] = s;
    }
}

// one thread per (c, k): the workgroups' partials in ascending order, in double
__global__ __launch_bounds__(256) void vp_join_grads_kernel(const float *__restrict__ partial, int nwg, int C,
                                                            float *__restrict__ dA, float *__restrict__ db) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= C * 4) return;
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += (double)partial[(size_t)w * C * 4 + e];
    const int c = e >> 2, k = e & 3;
    if (k == 3) db[c] = (float)s;
    else dA[c * 3 + k] = (float)s;
}

int v2p_launch(const int32_t *indices, int N, const int32_t *num_rows, int32_t *map, int B, int Z, int Y, int X, int clear,
               void *stream) {
    if (N < 0 || B <= 0 || Z <= 0 || Y <= 0 || X <= 0) return PCD_ERR_INVALID_ARG;
    if (N == 0) return PCD_OK;
    if (!indices || !map) return PCD_ERR_INVALID_ARG;
    v2p_kernel<<<pcd_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(indices, N, num_rows, map, B, Z, Y, X, clear);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

}  // namespace

extern "C" int pcd_voxel2pinds_scatter(const int32_t *indices, int N, const int32_t *num_rows, int32_t *map, int B, int Z, int Y,
                                       int X, void *stream) {
    PCD_ENTER();
    return v2p_launch(indices, N, num_rows, map, B, Z, Y, X, 0, stream);
}

extern "C" int pcd_voxel2pinds_clear(const int32_t *indices, int N, const int32_t *num_rows, int32_t *map, int B, int Z, int Y,
                                     int X, void *stream) {
    PCD_ENTER();
    return v2p_launch(indices, N, num_rows, map, B, Z, Y, X, 1, stream);
}

extern "C" int pcd_voxel_pool_query(int M, int N, int B, int Z, int Y, int X, int nsample, float radius, int z_range,
                                    int y_range, int x_range, const float *new_xyz, const float *xyz,
                                    const int32_t *new_coords, const int32_t *map, int32_t *idx, int32_t *cnt, double *partial,
                                    double *moments, void *stream) {
    PCD_ENTER();
    if (M < 0 || N < 0 || B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || nsample <= 0 || z_range < 0 || y_range < 0 || x_range < 0)
        return PCD_ERR_INVALID_ARG;
    if (nsample > PCD_VOXEL_POOL_MAX_NSAMPLE || z_range > 64 || y_range > 64 || x_range > 64) return PCD_ERR_UNSUPPORTED;
    if (!moments) return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nwg = pcd_div_up(M, VP_QPB);
    if (M > 0) {
        if (!new_xyz || !new_coords || !map || !idx || !cnt || !partial || (N > 0 && !xyz)) return PCD_ERR_INVALID_ARG;
        vp_query_kernel<<<nwg, 256, 0, st>>>(M, N, B, Z, Y, X, nsample, radius, z_range, y_range, x_range, new_xyz, xyz,
                                             new_coords, map, idx, cnt, partial);
    }
    vp_join_moments_kernel<<<1, 576, 0, st>>>(partial, nwg, moments);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_voxel_pool_fwd(int M, int N, int C, int nsample, const float *fin, const float *A, const float *b,
                                  const float *xyz, const float *new_xyz, const int32_t *idx, const int32_t *cnt, float *out,
                                  unsigned char *arg, void *stream) {
    PCD_ENTER();
    if (M < 0 || N < 0 || C <= 0 || nsample <= 0) return PCD_ERR_INVALID_ARG;
    if (C > PCD_VOXEL_POOL_MAX_C || nsample > PCD_VOXEL_POOL_MAX_NSAMPLE) return PCD_ERR_UNSUPPORTED;
    if (M == 0) return PCD_OK;
    if (!A || !b || !new_xyz || !idx || !cnt || !out || !arg || (N > 0 && (!fin || !xyz))) return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (C <= 32)
        vp_fwd_kernel<32><<<pcd_div_up(M, 8), 256, 0, st>>>(M, N, C, nsample, fin, A, b, xyz, new_xyz, idx, cnt, out, arg);
    else
        vp_fwd_kernel<64><<<pcd_div_up(M, 4), 256, 0, st>>>(M, N, C, nsample, fin, A, b, xyz, new_xyz, idx, cnt, out, arg);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_voxel_pool_bwd(int M, int N, int C, int nsample, const float *g, const float *out, const unsigned char *arg,
                                  const float *xyz, const float *new_xyz, const int32_t *idx, const int32_t *cnt,
                                  float *d_fin_zeroed, float *partial, float *dA, float *db, void *stream) {
    PCD_ENTER();
    if (M < 0 || N < 0 || C <= 0 || nsample <= 0) return PCD_ERR_INVALID_ARG;
    if (C > PCD_VOXEL_POOL_MAX_C || nsample > PCD_VOXEL_POOL_MAX_NSAMPLE) return PCD_ERR_UNSUPPORTED;
    if (!dA || !db) return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nwg = pcd_div_up(M, VP_BWD_QPB);
    if (M > 0) {
        if (!g || !out || !arg || !new_xyz || !idx || !cnt || !partial || (N > 0 && (!xyz || !d_fin_zeroed)))
            return PCD_ERR_INVALID_ARG;
        if (C <= 32)
            vp_bwd_kernel<32><<<nwg, 256, (size_t)8 * C * 4 * sizeof(float), st>>>(M, N, C, nsample, g, out, arg, xyz, new_xyz, idx,
                                                                                  cnt, d_fin_zeroed, partial);
        else
            vp_bwd_kernel<64><<<nwg, 256, (size_t)4 * C * 4 * sizeof(float), st>>>(M, N, C, nsample, g, out, arg, xyz, new_xyz, idx,
                                                                                  cnt, d_fin_zeroed, partial);
    }
    vp_join_grads_kernel<<<pcd_div_up(C * 4, 256), 256, 0, st>>>(partial, nwg, C, dA, db);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
