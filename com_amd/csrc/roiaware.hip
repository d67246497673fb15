// The reference's roiaware_pool3d package on the device (gfx950).  C ABI: include/pcd_ops.h (f5).  The point heads' targets,
// losses and decoding, which share the point-in-box geometry (roiaware_geom.h), are in pointhead.hip.
//
//   pcd_points_in_boxes_host     pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-168 (points_in_boxes_cpu): HOST
//                                pointers, no GPU call -- what box_utils.remove_points_in_boxes3d (box_utils.py:117-131)
//                                calls per frame inside the DataLoader workers of COMAug's database samplers
//   pcd_points_in_boxes          roiaware_pool3d_kernel.cu:16-36, :313-359 (points_in_boxes_gpu)
//   pcd_roiaware_pool3d_forward / _backward   roiaware_pool3d_kernel.cu:39-310
//
// Point-in-box: one thread per point; the frame's boxes are staged once per workgroup in LDS as centre, half height,
// cos / sin and the two double thresholds (roiaware_geom.h), in chunks of 128 (no cap on the number of boxes).  Every lane
// reads the same box (an LDS broadcast), the sincos is paid per box and workgroup instead of per (point, box) pair, and a
// lane stops at its first hit.
//
// RoI-aware pooling: the contract is the ORDER of a voxel's point list (ascending point index, cut after
// max_pts_each_voxel - 1 entries: what the reference's serial one-thread-per-box loop produces).  One workgroup per RoI
// walks the points 1024 at a time: all four waves test their points and leave a voxel id (or -1) per point in LDS, then
// wave 0 walks those ids in order and appends them, the rank of a point among the lanes with the same voxel coming from
// ballots, the voxel counters living in LDS.  The (N, P) int mask of the reference is never materialised.  Pooling and
// its backward run with the CHANNEL as the fastest thread index: a wave reads / adds into contiguous runs of one point's
// row (the lesson of pcd_group_points_stack_grad) instead of 64 different rows.
#include "common.h"
#include "roiaware_geom.h"

#define RA_COLLECT_PTS 1024     // points per pass of the collect kernel (4 per thread)
#define RA_MAX_VOXELS 8192      // voxel counters of one RoI in LDS (32 KiB)

namespace {

__global__ __launch_bounds__(256) void ra_points_in_boxes_kernel(const float *__restrict__ boxes, const float *__restrict__ pts,
                                                                 int nb, int np, int *__restrict__ out) {
    __shared__ RaBox s_box[RA_CHUNK];
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool valid = n < np;
    float x = 0.f, y = 0.f, z = 0.f;
    if (valid) {
        const float *p = pts + ((size_t)b * np + n) * 3;
        x = p[0];
        y = p[1];
        z = p[2];
    }
    int found = -1;
    for (int m0 = 0; m0 < nb; m0 += RA_CHUNK) {
        const int cnt = min(RA_CHUNK, nb - m0);
        __syncthreads();
        if ((int)threadIdx.x < cnt) s_box[threadIdx.x] = ra_prepare(boxes + ((size_t)b * nb + m0 + threadIdx.x) * 7, RA_MARGIN_DEVICE);
        __syncthreads();
        if (!valid || found >= 0) continue;
        for (int j = 0; j < cnt; ++j) {
            float lx, ly;
            if (ra_point_in_box(s_box[j], x, y, z, lx, ly)) {
                found = m0 + j;
                break;
            }
        }
    }
    if (valid) out[(size_t)b * np + n] = found;
}

// ---------------------------------------------------------------------------------------------------------------------
// RoI-aware pooling
__global__ __launch_bounds__(256) void ra_collect_kernel(const float *__restrict__ rois, const float *__restrict__ pts, int np, int ox,
                                                         int oy, int oz, int mpv, int *__restrict__ lists) {
    extern __shared__ int s_cnt[];                    // [ox * oy * oz]
    __shared__ int s_vox[RA_COLLECT_PTS];
    const int roi = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int nvox = ox * oy * oz;
    const float *r = rois + (size_t)roi * 7;
    const RaBox box = ra_prepare(r, RA_MARGIN_DEVICE);
    const float dx = r[3], dy = r[4], dz = r[5];
    const float x_res = __fdiv_rn(dx, (float)ox), y_res = __fdiv_rn(dy, (float)oy), z_res = __fdiv_rn(dz, (float)oz);
    int *L = lists + (size_t)roi * nvox * mpv;
    for (int v = tid; v < nvox; v += 256) s_cnt[v] = 0;
    const u64 lower = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int base = 0; base < np; base += RA_COLLECT_PTS) {
#pragma unroll
        for (int j = 0; j < RA_COLLECT_PTS / 256; ++j) {
            const int k = base + j * 256 + tid;
            int v = -1;
            if (k < np) {
                const float x = pts[(size_t)k * 3], y = pts[(size_t)k * 3 + 1], z = pts[(size_t)k * 3 + 2];
                float lx, ly;
                if (ra_point_in_box(box, x, y, z, lx, ly)) {
                    const float lz = z - box.cz;
                    v = (ra_voxel_index(lx, dx, x_res, ox) * oy + ra_voxel_index(ly, dy, y_res, oy)) * oz +
                        ra_voxel_index(lz, dz, z_res, oz);
                }
            }
            s_vox[j * 256 + tid] = v;
        }
        __syncthreads();
        if (tid < 64) {
            // wave 0 appends in point order: within a 64-point piece the lanes of one voxel are ranked by ballots
            for (int k0 = 0; k0 < RA_COLLECT_PTS; k0 += 64) {
                const int v = s_vox[k0 + lane];
                u64 act = __ballot(v >= 0);
                while (act) {
                    const int leader = __ffsll((long long)act) - 1;
                    const int lv = __shfl(v, leader, 64);
                    const u64 same = __ballot(v == lv);
                    const int have = s_cnt[lv];
                    if (v == lv) {
                        const int pos = have + __popcll(same & lower);
                        if (pos < mpv - 1) L[(size_t)lv * mpv + pos + 1] = base + k0 + lane;
                    }
                    if (lane == leader) s_cnt[lv] = min(have + __popcll(same), mpv - 1);
                    act &= ~same;
                }
            }
        }
        __syncthreads();
    }
    for (int v = tid; v < nvox; v += 256) L[(size_t)v * mpv] = s_cnt[v];
}

// one thread per (voxel, channel), channel fastest
template <bool AVG>
__global__ __launch_bounds__(256) void ra_pool_kernel(const float *__restrict__ feat, const int *__restrict__ lists, int nvox, int C,
                                                      int mpv, int np, float *__restrict__ pooled, int *__restrict__ argmax) {
    const int roi = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nvox * C) return;
    const int v = (int)(i / C), c = (int)(i - (size_t)v * C);
    const int *L = lists + ((size_t)roi * nvox + v) * mpv;
    const int total = min(L[0], mpv - 1);
    const size_t o = (size_t)roi * nvox * C + i;
    if (AVG) {
        float sum = 0.f;
        for (int k = 1; k <= total; ++k) {
            const int idx = L[k];
            if ((unsigned)idx < (unsigned)np) sum += feat[(size_t)idx * C + c];
        }
        pooled[o] = total > 0 ? __fdiv_rn(sum, (float)total) : 0.f;
    } else {
        int arg = -1;
        float mx = -INFINITY;                                            // (float)-1e50
        for (int k = 1; k <= total; ++k) {
            const int idx = L[k];
            if ((unsigned)idx >= (unsigned)np) continue;
            const float f = feat[(size_t)idx * C + c];
            if (f > mx) {                                                // the first strict maximum in list order
                mx = f;
                arg = idx;
            }
        }
        pooled[o] = arg != -1 ? mx : 0.f;
        argmax[o] = arg;
    }
}

// Backward, same thread layout: the lanes of a wave are consecutive channels of one voxel (C >= 64), so one atomic
// instruction adds into contiguous runs of at most as many point rows as the voxel holds (avg: exactly one row).
template <bool AVG>
__global__ __launch_bounds__(256) void ra_pool_grad_kernel(const int *__restrict__ lists, const int *__restrict__ argmax,
                                                           const float *__restrict__ grad_out, int nvox, int C, int mpv, int np,
                                                           float *__restrict__ grad_in) {
    const int roi = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nvox * C) return;
    const int v = (int)(i / C), c = (int)(i - (size_t)v * C);
    const size_t o = (size_t)roi * nvox * C + i;
    if (AVG) {
        const int *L = lists + ((size_t)roi * nvox + v) * mpv;
        const int total = min(L[0], mpv - 1);
        if (total <= 0) return;
        const float g = grad_out[o] * __fdiv_rn(1.f, fmaxf((float)total, 1.f));
        for (int k = 1; k <= total; ++k) {
            const int idx = L[k];
            if ((unsigned)idx < (unsigned)np) atomicAdd(grad_in + (size_t)idx * C + c, g);
        }
    } else {
        const int a = argmax[o];
        if ((unsigned)a < (unsigned)np) atomicAdd(grad_in + (size_t)a * C + c, grad_out[o]);
    }
}

bool pool_shape_ok(int num_rois, int ox, int oy, int oz, int channels, int mpv) {
    if (num_rois < 0 || ox < 1 || oy < 1 || oz < 1 || channels < 1 || mpv < 2) return false;
    if (ox > 255 || oy > 255 || oz > 255 || num_rois > 65535) return false;                   // (the reference: < 256)
    const long long nvox = (long long)ox * oy * oz;
    return nvox <= RA_MAX_VOXELS && nvox * channels < (1ll << 31) && nvox * mpv < (1ll << 31);
}

}  // namespace

extern "C" int pcd_points_in_boxes_host(const float *boxes_host, int num_boxes, const float *pts_host, int num_pts,
                                        int *out_host) {
    if (num_boxes < 0 || num_pts < 0) return PCD_ERR_INVALID_ARG;
    if (num_boxes == 0 || num_pts == 0) return PCD_OK;
    if (!boxes_host || !pts_host || !out_host) return PCD_ERR_INVALID_ARG;
    for (int i = 0; i < num_boxes; ++i) {
        const RaBox b = ra_prepare(boxes_host + (size_t)i * 7, RA_MARGIN_HOST);
        for (int j = 0; j < num_pts; ++j) {
            const float *p = pts_host + (size_t)j * 3;
            float lx, ly;
            out_host[(size_t)i * num_pts + j] = ra_point_in_box(b, p[0], p[1], p[2], lx, ly) ? 1 : 0;
        }
    }
    return PCD_OK;
}

extern "C" int pcd_points_in_boxes(const float *boxes, const float *pts, int batch, int num_boxes, int num_pts,
                                   int *box_idx_of_pts, void *stream) {
    PCD_ENTER();
    if (batch < 0 || num_boxes < 0 || num_pts < 0) return PCD_ERR_INVALID_ARG;
    if (batch == 0 || num_pts == 0) return PCD_OK;
    if (!pts || !box_idx_of_pts || (num_boxes > 0 && !boxes)) return PCD_ERR_INVALID_ARG;
    if (batch > 65535 || (long long)batch * num_pts * 3 >= (1ll << 31) || (long long)batch * num_boxes * 7 >= (1ll << 31))
        return PCD_ERR_UNSUPPORTED;
    dim3 grid((unsigned)pcd_div_up(num_pts, 256), (unsigned)batch);
    ra_points_in_boxes_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(boxes, pts, num_boxes, num_pts, box_idx_of_pts);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_roiaware_pool3d_forward(const float *rois, int num_rois, const float *pts, int num_pts,
                                           const float *pts_feature, int channels, int out_x, int out_y, int out_z,
                                           int max_pts_each_voxel, int pool_method, int *pts_idx_of_voxels, int *argmax,
                                           float *pooled_features, void *stream) {
    PCD_ENTER();
    if (num_pts < 0 || (pool_method != 0 && pool_method != 1)) return PCD_ERR_INVALID_ARG;
    if (!pool_shape_ok(num_rois, out_x, out_y, out_z, channels, max_pts_each_voxel) || (long long)num_pts * channels >= (1ll << 31))
        return PCD_ERR_UNSUPPORTED;
    if (num_rois == 0) return PCD_OK;
    if (!rois || !pts_idx_of_voxels || !pooled_features || (pool_method == 0 && !argmax) || (num_pts > 0 && (!pts || !pts_feature)))
        return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nvox = out_x * out_y * out_z;
    pcd_fill(pts_idx_of_voxels, 0, (size_t)num_rois * nvox * max_pts_each_voxel * sizeof(int), st);
    ra_collect_kernel<<<num_rois, 256, (size_t)nvox * sizeof(int), st>>>(rois, pts, num_pts, out_x, out_y, out_z, max_pts_each_voxel,
                                                                         pts_idx_of_voxels);
    dim3 grid((unsigned)(((size_t)nvox * channels + 255) / 256), (unsigned)num_rois);
    if (pool_method == 0)
        ra_pool_kernel<false><<<grid, 256, 0, st>>>(pts_feature, pts_idx_of_voxels, nvox, channels, max_pts_each_voxel, num_pts,
                                                    pooled_features, argmax);
    else
        ra_pool_kernel<true><<<grid, 256, 0, st>>>(pts_feature, pts_idx_of_voxels, nvox, channels, max_pts_each_voxel, num_pts,
                                                   pooled_features, nullptr);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_roiaware_pool3d_backward(const int *pts_idx_of_voxels, const int *argmax, const float *grad_out, int num_rois,
                                            int out_x, int out_y, int out_z, int channels, int max_pts_each_voxel,
                                            int pool_method, int num_pts, float *grad_in, void *stream) {
    PCD_ENTER();
    if (num_pts < 0 || (pool_method != 0 && pool_method != 1)) return PCD_ERR_INVALID_ARG;
    if (!pool_shape_ok(num_rois, out_x, out_y, out_z, channels, max_pts_each_voxel) || (long long)num_pts * channels >= (1ll << 31))
        return PCD_ERR_UNSUPPORTED;
    if (num_pts == 0) return PCD_OK;
    if (!grad_in) return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    pcd_fill(grad_in, 0, (size_t)num_pts * channels * sizeof(float), st);
    if (num_rois > 0) {
        if (!grad_out || (pool_method == 0 ? !argmax : !pts_idx_of_voxels)) return PCD_ERR_INVALID_ARG;
        const int nvox = out_x * out_y * out_z;
        dim3 grid((unsigned)(((size_t)nvox * channels + 255) / 256), (unsigned)num_rois);
        if (pool_method == 0)
            ra_pool_grad_kernel<false><<<grid, 256, 0, st>>>(pts_idx_of_voxels, argmax, grad_out, nvox, channels, max_pts_each_voxel,
                                                             num_pts, grad_in);
        else
            ra_pool_grad_kernel<true><<<grid, 256, 0, st>>>(pts_idx_of_voxels, argmax, grad_out, nvox, channels, max_pts_each_voxel,
                                                            num_pts, grad_in);
    }
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
