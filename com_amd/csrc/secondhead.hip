// SECONDHead, the IoU-rectification RoI head of SECOND-IoU, on the device (gfx950).  C ABI: include/pcd_ops.h (f7).
//
//   pcd_bev_roi_grid_pool              pcdet/models/roi_heads/second_head.py:63-120 (roi_grid_pool: per-frame affine_grid +
//                                      grid_sample, align_corners=True, bilinear, zero padding) for the whole batch
//   pcd_second_head_iou_loss_forward / _backward   second_head.py:163-188 (get_box_iou_layer_loss)
//   pcd_points_in_boxes_count          pcdet/models/detectors/second_net_iou.py:133-138 (points_in_boxes_cpu(...).sum(dim=1)
//                                      per frame, the host margin of roiaware_pool3d.cpp:131)
//
// Pooling: one workgroup per (RoI, chunk of SP_CHUNK channels).  The G * G sample records (the floor pixel, clamped into
// [-1, W - 1] x [-1, H - 1], and the two fractions) are computed once into LDS: no theta, no grid tensor, no expanded view of
// the map.  A neighbour outside the map is never read (its load is predicated, the value is 0).  Two thread layouts, one
// arithmetic (so both write the same bits):
//   * channels-last map (channel stride 1): lanes run along c -- the 64 channels of a corner are one contiguous run -- and the
//     chunk goes through a padded LDS tile [c][G * G + 1], so that the [c0 * G * G, (c0 + chunk) * G * G) output range is
//     written as one contiguous run too;
//   * any other strides (NCHW): lanes run along the samples of a channel plane and write straight to the output.
// The pooled features feed detached FC layers in the reference (second_head.py:74-75): there is no backward.
//
// Loss: one workgroup, thread t sums rows t, t + 256, ... in fp64, a fixed tree joins them: bit-reproducible.
//
// Counts: one thread per point; the boxes of the frames a workgroup's points belong to are staged in LDS in chunks of
// SC_CHUNK (as ra_points_in_boxes_kernel stages them) beside one LDS counter per box; integer atomics only, LDS first, then
// one global add per workgroup and box that was hit.
#include "common.h"
#include "roiaware_geom.h"

#include <math.h>

#define SP_CHUNK 64                         // channels per workgroup
#define SP_MAX_G PCD_SECOND_POOL_MAX_G
#define SP_MAX_S (SP_MAX_G * SP_MAX_G)      // samples of a RoI
#define SC_CHUNK 128                        // boxes staged per pass

namespace {

struct SpCfg {
    int N, C, H, W, G, dtype;
    long long sb, sc, sy, sx;               // strides of the map in elements
    long long roi_stride;
    float min_x, min_y, cell_x, cell_y;
};

struct SpSample {
    int x0, y0;                             // floor(ix), floor(iy) clamped into [-1, W - 1] / [-1, H - 1]
    float fx, fy;                           // ix - floor(ix), iy - floor(iy); 0 weights for a sample off the map
    int live;                               // 0: every neighbour is off the map (or the coordinates are not finite)
};

// sample (i, j) of the RoI, second_head.py:87-113 collapsed: centre and half extents in pixels, rotated by the heading
__device__ __forceinline__ SpSample sp_sample(const SpCfg &c, const float *roi, int p) {
    const int i = p / c.G, j = p - i * c.G;
    const float cx = __fdiv_rn(roi[0] - c.min_x, c.cell_x), cy = __fdiv_rn(roi[1] - c.min_y, c.cell_y);
    const float hx = __fdiv_rn(roi[3] * 0.5f, c.cell_x), hy = __fdiv_rn(roi[4] * 0.5f, c.cell_y);
    float sa, ca;
    sincosf(roi[6], &sa, &ca);
    const float u = __fdiv_rn((float)(2 * j), (float)(c.G - 1)) - 1.f, v = __fdiv_rn((float)(2 * i), (float)(c.G - 1)) - 1.f;
    const float ix = cx + hx * (ca * u - sa * v), iy = cy + hy * (sa * u + ca * v);
    const float flx = floorf(ix), fly = floorf(iy);
    SpSample s;
    // (comparisons in float before any conversion: false for NaN, safe for values beyond the int range)
    s.live = (flx >= -1.f && flx <= (float)(c.W - 1) && fly >= -1.f && fly <= (float)(c.H - 1)) ? 1 : 0;
    s.x0 = s.live ? (int)flx : -1;
    s.y0 = s.live ? (int)fly : -1;
    s.fx = s.live ? ix - flx : 0.f;
    s.fy = s.live ? iy - fly : 0.f;
    return s;
}

// the bilinear value of one channel at one sample: the four neighbours in a fixed order, each read only when inside the map
__device__ __forceinline__ float sp_value(const SpCfg &c, const void *feat, long long base, const SpSample &s) {
    if (!s.live) return 0.f;
    const bool xl = s.x0 >= 0, xr = s.x0 + 1 < c.W, yt = s.y0 >= 0, yb = s.y0 + 1 < c.H;
    // (rows and columns clamped into the map: an address that is formed is a valid one, whether it is read or not)
    const long long r0 = base + (long long)(yt ? s.y0 : 0) * c.sy, r1 = base + (long long)(yb ? s.y0 + 1 : 0) * c.sy;
    const long long q0 = (long long)(xl ? s.x0 : 0) * c.sx, q1 = (long long)(xr ? s.x0 + 1 : 0) * c.sx;
    const float f00 = (yt && xl) ? load_el(feat, c.dtype, r0 + q0) : 0.f;
    const float f01 = (yt && xr) ? load_el(feat, c.dtype, r0 + q1) : 0.f;
    const float f10 = (yb && xl) ? load_el(feat, c.dtype, r1 + q0) : 0.f;
    const float f11 = (yb && xr) ? load_el(feat, c.dtype, r1 + q1) : 0.f;
    const float wx1 = s.fx, wx0 = 1.f - s.fx, wy1 = s.fy, wy0 = 1.f - s.fy;
    return ((f00 * (wx0 * wy0) + f01 * (wx1 * wy0)) + f10 * (wx0 * wy1)) + f11 * (wx1 * wy1);
}

// CLAST: the map's channel stride is 1
template <bool CLAST>
__global__ __launch_bounds__(256) void sp_pool_kernel(SpCfg c, const void *__restrict__ feat, const float *__restrict__ rois,
                                                      void *__restrict__ out) {
    extern __shared__ float s_tile[];       // CLAST: [SP_CHUNK][G * G + 1]
    __shared__ SpSample s_rec[SP_MAX_S];
    const int GG = c.G * c.G;
    const long long r = blockIdx.y;         // RoI b * N + n
    const int c0 = blockIdx.x * SP_CHUNK;
    const int cn = min(SP_CHUNK, c.C - c0);
    const float *roi = rois + r * c.roi_stride;
    if ((int)threadIdx.x < GG) s_rec[threadIdx.x] = sp_sample(c, roi, threadIdx.x);
    __syncthreads();
    const long long fbase = (r / c.N) * c.sb;
    const long long obase = (r * c.C + c0) * (long long)GG;
    if (CLAST) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int ld = GG + 1;
        if (lane < cn) {
            const long long base = fbase + (long long)(c0 + lane) * c.sc;
            for (int p = wave; p < GG; p += 4) s_tile[lane * ld + p] = sp_value(c, feat, base, s_rec[p]);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cn * GG; e += 256) {
            const int ch = e / GG, p = e - ch * GG;
            store_el(out, c.dtype, obase + e, s_tile[ch * ld + p]);
        }
    } else {
        for (int e = threadIdx.x; e < cn * GG; e += 256) {
            const int ch = e / GG, p = e - ch * GG;
            store_el(out, c.dtype, obase + e, sp_value(c, feat, fbase + (long long)(c0 + ch) * c.sc, s_rec[p]));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// get_box_iou_layer_loss
template <bool GRAD>
__device__ __forceinline__ float sh_loss_el(int kind, float x, float t) {
    if (kind == PCD_SECOND_IOU_LOSS_BCE) {
        // binary_cross_entropy_with_logits, the stable form: max(x, 0) - x t + log(1 + exp(-|x|)); d / dx = sigmoid(x) - t
        if (!GRAD) return (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x)));
        return sigmoid_f32(x) - t;
    }
    const float diff = x - t;
    if (kind == PCD_SECOND_IOU_LOSS_L2) return GRAD ? 2.f * diff : diff * diff;
    const float beta = 1.0f / 9.0f, n = fabsf(diff);                         // loss_utils.py:363-370
    if (!GRAD) return n < beta ? 0.5f * n * n / beta : n - 0.5f * beta;
    return n < beta ? diff / beta : (diff > 0.f ? 1.f : -1.f);
}

__global__ __launch_bounds__(256) void sh_loss_forward_kernel(const void *__restrict__ logits, int dtype, long long stride,
                                                              const float *__restrict__ labels, int n, int kind, float weight,
                                                              float *__restrict__ out) {
    __shared__ double s[2][256];
    double a0 = 0.0, a1 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float t = labels[i];
        if (t >= 0.f) {
            a0 += (double)sh_loss_el<false>(kind, load_el(logits, dtype, (long long)i * stride), t);
            a1 += 1.0;
        }
    }
    s[0][threadIdx.x] = a0;
    s[1][threadIdx.x] = a1;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s[0][threadIdx.x] += s[0][threadIdx.x + d];
            s[1][threadIdx.x] += s[1][threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)(s[0][0] / fmax(s[1][0], 1.0)) * weight;
        out[1] = (float)s[1][0];
    }
}

__global__ __launch_bounds__(256) void sh_loss_backward_kernel(const void *__restrict__ logits, int dtype, long long stride,
                                                               const float *__restrict__ labels, int n, int kind, float weight,
                                                               const float *__restrict__ fwd_out, const float *__restrict__ grad_out,
                                                               void *__restrict__ d_logits) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float t = labels[i];
    float d = 0.f;
    if (t >= 0.f)
        d = sh_loss_el<true>(kind, load_el(logits, dtype, (long long)i * stride), t) *
            __fdiv_rn(grad_out[0] * weight, fmaxf(fwd_out[1], 1.f));
    store_el(d_logits, dtype, (long long)i * stride, d);
}

// ---------------------------------------------------------------------------------------------------------------------
// points inside each box
__global__ __launch_bounds__(256) void sc_count_kernel(const float *__restrict__ points, int np, const float *__restrict__ boxes,
                                                       int batch, int nb, int *__restrict__ counts) {
    __shared__ RaBox s_box[SC_CHUNK];
    __shared__ int s_cnt[SC_CHUNK];
    __shared__ int s_lo, s_hi;
    const int n = blockIdx.x * 256 + threadIdx.x;
    int frame = -1;
    float x = 0.f, y = 0.f, z = 0.f;
    if (n < np) {
        const float *p = points + (size_t)n * 4;
        const float bf = p[0];
        if (bf >= 0.f && bf < (float)batch) frame = (int)bf;               // (false for NaN; rows of no frame count nowhere)
        x = p[1];
        y = p[2];
        z = p[3];
    }
    if (threadIdx.x == 0) {
        s_lo = batch;
        s_hi = -1;
    }
    __syncthreads();
    if (frame >= 0) {
        atomicMin(&s_lo, frame);
        atomicMax(&s_hi, frame);
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;
    for (int b = lo; b <= hi; ++b) {
        for (int m0 = 0; m0 < nb; m0 += SC_CHUNK) {
            const int cnt = min(SC_CHUNK, nb - m0);
            __syncthreads();
            if ((int)threadIdx.x < cnt) {
                s_box[threadIdx.x] = ra_prepare(boxes + ((size_t)b * nb + m0 + threadIdx.x) * 7, RA_MARGIN_HOST);
                s_cnt[threadIdx.x] = 0;
            }
            __syncthreads();
            if (frame == b) {
                for (int j = 0; j < cnt; ++j) {
                    float lx, ly;
                    if (ra_point_in_box(s_box[j], x, y, z, lx, ly)) atomicAdd(&s_cnt[j], 1);
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < cnt && s_cnt[threadIdx.x] > 0)
                atomicAdd(&counts[(size_t)b * nb + m0 + threadIdx.x], s_cnt[threadIdx.x]);
        }
    }
}

}  // namespace

extern "C" int pcd_bev_roi_grid_pool(const void *features, int dtype, int batch, int channels, int height, int width,
                                     long long stride_b, long long stride_c, long long stride_y, long long stride_x,
                                     const float *rois, int num_rois, long long roi_stride, int grid_size, float min_x,
                                     float min_y, float cell_x, float cell_y, void *pooled, void *stream) {
    PCD_ENTER();
    if (batch < 0 || num_rois < 0 || channels < 1 || (dtype != PCD_F32 && dtype != PCD_BF16)) return PCD_ERR_INVALID_ARG;
    if (grid_size < 2 || grid_size > SP_MAX_G || height < 2 || width < 2) return PCD_ERR_UNSUPPORTED;
    if (!(cell_x > 0.f) || !(cell_y > 0.f) || roi_stride < 7) return PCD_ERR_INVALID_ARG;
    if (stride_b < 0 || stride_c < 1 || stride_y < 1 || stride_x < 1) return PCD_ERR_INVALID_ARG;
    if (batch == 0 || num_rois == 0) return PCD_OK;
    if (!features || !rois || !pooled) return PCD_ERR_INVALID_ARG;
    if ((long long)batch * num_rois > 65535 || (long long)height * width >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
    SpCfg c;
    c.N = num_rois, c.C = channels, c.H = height, c.W = width, c.G = grid_size, c.dtype = dtype;
    c.sb = stride_b, c.sc = stride_c, c.sy = stride_y, c.sx = stride_x, c.roi_stride = roi_stride;
    c.min_x = min_x, c.min_y = min_y, c.cell_x = cell_x, c.cell_y = cell_y;
    dim3 grid((unsigned)pcd_div_up(channels, SP_CHUNK), (unsigned)(batch * num_rois));
    if (stride_c == 1 && channels > 1) {
        const size_t lds = (size_t)SP_CHUNK * (grid_size * grid_size + 1) * sizeof(float);
        // G = 16: 64.25 KiB of tile, above the default limit of a launch.  The attribute belongs to the CURRENT device, so
        // it is set at every such call (a host-side setting, no stream work: legal under capture) and nothing is cached.
        if (lds > 48 * 1024 &&
            hipFuncSetAttribute((const void *)sp_pool_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((size_t)SP_CHUNK * (SP_MAX_S + 1) * sizeof(float))) != hipSuccess)
            return PCD_ERR_UNSUPPORTED;
        sp_pool_kernel<true><<<grid, 256, lds, (hipStream_t)stream>>>(c, features, rois, pooled);
    } else {
        sp_pool_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(c, features, rois, pooled);
    }
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

static bool sh_loss_args_ok(const void *logits, int dtype, long long stride, const float *labels, int n, int kind) {
    return logits && labels && n >= 1 && stride >= 1 && (dtype == PCD_F32 || dtype == PCD_BF16) &&
           (kind == PCD_SECOND_IOU_LOSS_BCE || kind == PCD_SECOND_IOU_LOSS_L2 || kind == PCD_SECOND_IOU_LOSS_SMOOTH_L1);
}

extern "C" int pcd_second_head_iou_loss_forward(const void *logits, int dtype, long long stride, const float *labels, int n,
                                                int kind, float weight, float *out, void *stream) {
    PCD_ENTER();
    if (!sh_loss_args_ok(logits, dtype, stride, labels, n, kind) || !out) return PCD_ERR_INVALID_ARG;
    sh_loss_forward_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, dtype, stride, labels, n, kind, weight, out);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_second_head_iou_loss_backward(const void *logits, int dtype, long long stride, const float *labels, int n,
                                                 int kind, float weight, const float *out, const float *grad_out,
                                                 void *d_logits, void *stream) {
    PCD_ENTER();
    if (!sh_loss_args_ok(logits, dtype, stride, labels, n, kind) || !out || !grad_out || !d_logits) return PCD_ERR_INVALID_ARG;
    sh_loss_backward_kernel<<<pcd_div_up(n, 256), 256, 0, (hipStream_t)stream>>>(logits, dtype, stride, labels, n, kind, weight,
                                                                                 out, grad_out, d_logits);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_points_in_boxes_count(const float *points, int num_points, const float *boxes, int batch, int num_boxes,
                                         int *counts, void *stream) {
    PCD_ENTER();
    if (num_points < 0 || batch < 0 || num_boxes < 0) return PCD_ERR_INVALID_ARG;
    if (batch == 0 || num_boxes == 0) return PCD_OK;
    if (!counts || !boxes || (num_points > 0 && !points)) return PCD_ERR_INVALID_ARG;
    if ((long long)num_points * 4 >= (1ll << 31) || (long long)batch * num_boxes * 7 >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
    if (hipMemsetAsync(counts, 0, (size_t)batch * num_boxes * sizeof(int), (hipStream_t)stream) != hipSuccess) return PCD_ERR_LAUNCH;
    if (num_points == 0) return PCD_OK;
    sc_count_kernel<<<pcd_div_up(num_points, 256), 256, 0, (hipStream_t)stream>>>(points, num_points, boxes, batch, num_boxes, counts);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
