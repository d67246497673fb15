// Shared pieces of the CenterHead kernels (centerhead.hip: plain CenterHead; com_head.hip: the COM curriculum head).
#pragma once
#include <type_traits>

#include "common.h"

namespace {

struct AssignGeom {
    float range_x, range_y, vs_x, vs_y;
    int stride, W, H, num_max, min_radius, code, head_classes;
    float overlap;
    int cls_map[16];       // dataset class id (1-based; 0 = padding) -> 1-based id inside this head, 0 = not in the head
};

// centernet_utils.py:46-72 in float32, operation by operation
__device__ __forceinline__ float gaussian_radius_f32(float height, float width, float min_overlap) {
    const float a1 = 1.0f;
    const float b1 = height + width;
    const float c1 = width * height * (1.0f - min_overlap) / (1.0f + min_overlap);
    const float sq1 = sqrtf(b1 * b1 - 4.0f * a1 * c1);
    const float r1 = (b1 + sq1) / 2.0f;
    const float a2 = 4.0f;
    const float b2 = 2.0f * (height + width);
    const float c2 = (1.0f - min_overlap) * width * height;
    const float sq2 = sqrtf(b2 * b2 - 4.0f * a2 * c2);
    const float r2 = (b2 + sq2) / 2.0f;
    const float a3 = 4.0f * min_overlap;
    const float b3 = -2.0f * min_overlap * (height + width);
    const float c3 = (min_overlap - 1.0f) * width * height;
    const float sq3 = sqrtf(b3 * b3 - 4.0f * a3 * c3);
    const float r3 = (b3 + sq3) / 2.0f;
    return fminf(fminf(r1, r2), r3);
}

// 1-based class of ground-truth row r inside this head; 0 = padding, a class of another head, or r >= n
__device__ __forceinline__ int assign_class(const float *rows, int r, int n, const AssignGeom &G) {
    if (r >= n) return 0;
    const int cls = (int)rows[(size_t)r * G.code + G.code - 1];
    return (cls >= 0 && cls < 16) ? G.cls_map[cls] : 0;
}

// centre on the feature map, its pixel and the Gaussian radius of ground-truth row q (center_head.py:104-161)
struct AssignRow {
    float cx, cy;
    int ix, iy, radius;
    bool valid;                     // the box has an extent and its pixel is on the map
};
__device__ __forceinline__ AssignRow assign_row(const float *q, const AssignGeom &G) {
    AssignRow a;
    a.cx = (q[0] - G.range_x) / G.vs_x / (float)G.stride;
    a.cy = (q[1] - G.range_y) / G.vs_y / (float)G.stride;
    a.cx = fminf(fmaxf(a.cx, 0.0f), (float)G.W - 0.5f);
    a.cy = fminf(fmaxf(a.cy, 0.0f), (float)G.H - 0.5f);
    a.ix = (int)a.cx;
    a.iy = (int)a.cy;
    const float dx = q[3] / G.vs_x / (float)G.stride, dy = q[4] / G.vs_y / (float)G.stride;
    const int radius = (int)gaussian_radius_f32(dx, dy, G.overlap);
    a.radius = radius < G.min_radius ? G.min_radius : radius;
    a.valid = dx > 0.0f && dy > 0.0f && a.ix >= 0 && a.ix <= G.W && a.iy >= 0 && a.iy <= G.H;
    return a;
}
// the regression targets of the row: o[0 .. code)
__device__ __forceinline__ void encode_box(const float *q, const AssignRow &a, int code, float *o) {
    o[0] = a.cx - (float)a.ix;
    o[1] = a.cy - (float)a.iy;
    o[2] = q[2];
    o[3] = logf(q[3]);
    o[4] = logf(q[4]);
    o[5] = logf(q[5]);
    o[6] = cosf(q[6]);
    o[7] = sinf(q[6]);
    for (int j = 8; j < code; ++j) o[j] = q[j - 1];
}

// one wave per (batch, object): max the object's Gaussian into its class plane (centernet_utils.py:75-107)
__global__ __launch_bounds__(64) void draw_gaussian_kernel(const int4 *__restrict__ draw, AssignGeom G,
                                                           float *__restrict__ heatmap) {
    const size_t at = blockIdx.x;
    const int4 d = draw[at];
    if (d.x < 0) return;
    const int b = (int)(at / G.num_max);
    const int radius = d.w, x = d.y, y = d.z;
    const int left = min(x, radius), right = min(G.W - x, radius + 1);
    const int top = min(y, radius), bottom = min(G.H - y, radius + 1);
    const int w = left + right, h = top + bottom;
    if (w <= 0 || h <= 0) return;
    const double sigma = (double)(2 * radius + 1) / 6.0;
    const double eps_cut = 2.220446049250313e-16;             // np.finfo(float64).eps * h.max(), h.max() = 1
    int *plane = reinterpret_cast<int *>(heatmap + ((size_t)b * G.head_classes + d.x) * G.H * G.W);
    for (int p = threadIdx.x; p < w * h; p += 64) {
        const int py = p / w, px = p - py * w;
        const int gx = px - left, gy = py - top;               // offset from the centre
        double v = exp(-(double)(gx * gx + gy * gy) / (2.0 * sigma * sigma));
        if (v < eps_cut) v = 0.0;
        const float f = (float)v;
        atomicMax(plane + (size_t)(y + gy) * G.W + (x + gx), __float_as_int(f));
    }
}

constexpr int CHL_BLOCKS = 256;     // partial rows of the forward pass
constexpr int CHL_MAX_REG = 8;      // regression branches per head
constexpr int CHL_MAX_DIM = 16;     // code dimensions
constexpr int CHL_MAX_OBJS = 2048;  // objects per frame (num_max_objs; the reference uses 500): LDS list of the backward

struct ChlMap {                     // one prediction map [B][c][H][W] behind strides
    const void *p;
    void *g;                        // its gradient (same layout), backward only
    long long sb, sc, sh, sw;
    int c, dtype;                   // PCD_F32 / PCD_BF16
};
struct ChlRegs {
    ChlMap m[CHL_MAX_REG];
    int n, dims;                    // dims = sum of c
};

__device__ __forceinline__ long long chl_at(const ChlMap &m, int b, int c, int y, int x) {
    return b * m.sb + c * m.sc + y * m.sh + x * m.sw;
}
// where element e of a dense [B][C][H][W] walk lies in the map
__device__ __forceinline__ long long chl_at_linear(const ChlMap &m, unsigned e, int C, int H, int W) {
    const int x = (int)(e % (unsigned)W);
    unsigned t = e / (unsigned)W;
    const int y = (int)(t % (unsigned)H);
    t /= (unsigned)H;
    const int c = (int)(t % (unsigned)C), b = (int)(t / (unsigned)C);
    return chl_at(m, b, c, y, x);
}
__device__ __forceinline__ float chl_load(const ChlMap &m, long long off) { return load_el(m.p, m.dtype, off); }
__device__ __forceinline__ void chl_store_grad(const ChlMap &m, long long off, float v) { store_el(m.g, m.dtype, off, v); }

// The focal loss of both heads (loss_utils.py:611-643, :1178-1310) on p = clamp(sigmoid(x), 1e-4, 1 - 1e-4): the terms of
// a positive (g == 1) and of a negative (g < 1), and their derivatives in p.
__device__ __forceinline__ float focal_clamp(float s) { return fminf(fmaxf(s, 1e-4f), 1.0f - 1e-4f); }
__device__ __forceinline__ float chl_pred(const ChlMap &hm, long long off) {
    return focal_clamp(sigmoid_f32(chl_load(hm, off)));
}
__device__ __forceinline__ float focal_pos(float p) {
    const float q = 1.0f - p;
    return logf(p) * (q * q);
}
__device__ __forceinline__ float focal_neg(float p, float g) {
    const float w1 = 1.0f - g, w2 = w1 * w1;
    return logf(1.0f - p) * (p * p) * (w2 * w2);
}
__device__ __forceinline__ float focal_pos_grad(float p) {
    const float q = 1.0f - p;
    return q * q / p - 2.0f * q * logf(p);
}
__device__ __forceinline__ float focal_neg_grad(float p, float g) {
    const float w1 = 1.0f - g, w2 = w1 * w1;
    return (-(p * p) / (1.0f - p) + 2.0f * p * logf(1.0f - p)) * (w2 * w2);
}

__device__ __forceinline__ double chl_block_sum(double v, double *lds /*[4]*/) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return t;
}

// An object's weight in the regression loss: 0 / 1 from the CenterHead's int64 mask, the COM head's float box mask as it is
__device__ __forceinline__ float chl_mask_weight(long long m) { return m != 0 ? 1.0f : 0.0f; }
__device__ __forceinline__ float chl_mask_weight(float m) { return m; }

// Regression L1 partials of a forward kernel (256 threads): workgroup b < B takes the objects of frame b (a thread per
// object, all code dimensions: the gathers of one object are independent loads), every workgroup writes its row (zeros
// beyond the frames): row[0 .. dims) = sums of |pred * m - target * m| per code dimension, row[dims] = sum of m.
template <class MaskT>
__device__ __forceinline__ void chl_reg_partials(const ChlRegs &regs, int B, int W, const long long *__restrict__ ind,
                                                 const MaskT *__restrict__ mask, const float *__restrict__ target,
                                                 int M, double *__restrict__ row, double *lds /*[4]*/) {
    double acc[CHL_MAX_DIM + 1];
#pragma unroll
    for (int d = 0; d <= CHL_MAX_DIM; ++d) acc[d] = 0.0;
    if ((int)blockIdx.x < B) {
        const int b = blockIdx.x;
        for (int m0 = threadIdx.x; m0 < M; m0 += 256) {
            const int o = b * M + m0;
            const float mk = chl_mask_weight(mask[o]);
            const long long pix = ind[o];
            const int y = (int)(pix / W), x = (int)(pix % W);
            acc[CHL_MAX_DIM] += (double)mk;
            int d0 = 0;
            for (int r = 0; r < regs.n; ++r) {
                const ChlMap &m = regs.m[r];
                for (int c = 0; c < m.c; ++c) {
                    const float pr = chl_load(m, chl_at(m, b, c, y, x));
                    const float v = fabsf(pr * mk - target[(size_t)o * regs.dims + d0 + c] * mk);
#pragma unroll
                    for (int d = 0; d < CHL_MAX_DIM; ++d)      // (static register index)
                        if (d == d0 + c) acc[d] += (double)v;
                }
                d0 += m.c;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < CHL_MAX_DIM; ++d) {
        const double t = chl_block_sum(acc[d], lds);
        if (threadIdx.x == 0 && d < regs.dims) row[d] = t;
    }
    const double n = chl_block_sum(acc[CHL_MAX_DIM], lds);
    if (threadIdx.x == 0) row[regs.dims] = n;
}

// the backward kernels zero the regression gradients (grid-strided); chl_scatter_kernel then fills the object pixels
__device__ __forceinline__ void chl_zero_reg_grads(const ChlRegs &regs, int B, int H, int W) {
    for (int r = 0; r < regs.n; ++r) {
        const ChlMap &m = regs.m[r];
        const long long n = (long long)B * m.c * ((long long)H * W);
        for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < (unsigned)n; e += gridDim.x * 256u)
            chl_store_grad(m, chl_at_linear(m, e, m.c, H, W), 0.0f);
    }
}

// Regression gradients, a block per frame.  The masked objects are first compacted into LDS in object order (typically
// < 100 of the 500 slots); then one thread per object: the FIRST object of a pixel adds up the gradients of all objects
// of that pixel (in object order: no atomics, deterministic) and stores them.  MaskT = long long: the CenterHead's 0 / 1
// mask, d |pr - t| / d pr = sign(pr - t); float: the COM head's box mask, d |pr m - t m| / d pr = sign(pr m - t m) m.
template <class MaskT>
__global__ __launch_bounds__(256) void chl_scatter_kernel(ChlRegs regs, int W, const long long *__restrict__ ind,
                                                          const MaskT *__restrict__ mask,
                                                          const float *__restrict__ target, int M,
                                                          const float *__restrict__ code_weights,
                                                          const float *__restrict__ out,
                                                          const float *__restrict__ grad_out, float loc_weight) {
    __shared__ int pix_s[CHL_MAX_OBJS];
    __shared__ int obj_s[CHL_MAX_OBJS];
    __shared__ int lds[4];
    const int b = blockIdx.x;
    int K = 0;
    for (int base = 0; base < M; base += 256) {
        const int m0 = base + threadIdx.x;
        const bool on = m0 < M && mask[b * M + m0] != 0;
        int total;
        const int pos = K + block_exclusive_scan(on ? 1 : 0, lds, total);
        if (on && pos < CHL_MAX_OBJS) {
            pix_s[pos] = (int)ind[b * M + m0];
            obj_s[pos] = b * M + m0;
        }
        K += total;
    }
    __syncthreads();
    K = K < CHL_MAX_OBJS ? K : CHL_MAX_OBJS;
    const float scale = loc_weight / fmaxf(out[5], 1.0f) * grad_out[0];
    for (int k = threadIdx.x; k < K; k += 256) {
        const int pix = pix_s[k];
        bool first = true;
        for (int j = 0; j < k; ++j) first = first && pix_s[j] != pix;
        if (!first) continue;
        const int y = pix / W, x = pix - y * W;
        int d0 = 0;
        for (int r = 0; r < regs.n; ++r) {
            const ChlMap &mp = regs.m[r];
            for (int c = 0; c < mp.c; ++c) {
                const long long off = chl_at(mp, b, c, y, x);
                const float pr = chl_load(mp, off);
                float gsum = 0.0f;
                for (int j = k; j < K; ++j) {
                    if (pix_s[j] != pix) continue;
                    const float t = target[(size_t)obj_s[j] * regs.dims + d0 + c];
                    if constexpr (std::is_same<MaskT, float>::value) {
                        const float mk = mask[obj_s[j]];
                        const float diff = pr * mk - t * mk;
                        gsum += diff > 0.0f ? mk : (diff < 0.0f ? -mk : 0.0f);
                    } else {
                        const float diff = pr - t;
                        gsum += diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
                    }
                }
                chl_store_grad(mp, off, scale * code_weights[d0 + c] * gsum);
            }
            d0 += mp.c;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side of the entry points
static AssignGeom assign_geom(const float *range_xy, const float *voxel_size_xy, int feature_map_stride, int fm_w,
                              int fm_h, int num_max_objs, int min_radius, int code_size, int head_classes,
                              float gaussian_overlap, const int *class_map, int n_class_map) {
    AssignGeom G = {};
    G.range_x = range_xy[0]; G.range_y = range_xy[1];
    G.vs_x = voxel_size_xy[0]; G.vs_y = voxel_size_xy[1];
    G.stride = feature_map_stride; G.W = fm_w; G.H = fm_h; G.num_max = num_max_objs; G.min_radius = min_radius;
    G.code = code_size; G.head_classes = head_classes; G.overlap = gaussian_overlap;
    for (int i = 0; i < n_class_map; ++i) G.cls_map[i] = class_map[i];
    return G;
}

// What the four loss entry points check alike about the maps, and the maps as the kernels take them.  d_hm != NULL marks
// a backward pass, which needs a gradient pointer per regression map.
static int chl_pack(int batch, int C, int height, int width, const float *gt_heatmap, const float *out, const void *hm,
                    void *d_hm, int hm_dtype, const long long *hm_strides, const void *const *reg_ptrs,
                    void *const *reg_grads, const int *reg_channels, int reg_dtype, const long long *reg_strides,
                    int n_reg, ChlMap *H_, ChlRegs *R) {
    if (batch <= 0 || C <= 0 || height <= 0 || width <= 0 || !gt_heatmap || !out || (d_hm && n_reg > 0 && !reg_grads))
        return PCD_ERR_INVALID_ARG;
    if (!hm || !hm_strides || n_reg < 0 || n_reg > CHL_MAX_REG || (n_reg > 0 && (!reg_ptrs || !reg_channels || !reg_strides)))
        return PCD_ERR_INVALID_ARG;
    if ((hm_dtype != PCD_F32 && hm_dtype != PCD_BF16) || (reg_dtype != PCD_F32 && reg_dtype != PCD_BF16))
        return PCD_ERR_UNSUPPORTED;
    *H_ = ChlMap{hm, d_hm, hm_strides[0], hm_strides[1], hm_strides[2], hm_strides[3], C, hm_dtype};
    R->n = n_reg;
    R->dims = 0;
    for (int r = 0; r < n_reg; ++r) {
        if (!reg_ptrs[r] || reg_channels[r] <= 0) return PCD_ERR_INVALID_ARG;
        R->m[r] = ChlMap{reg_ptrs[r], reg_grads ? reg_grads[r] : nullptr, reg_strides[4 * r], reg_strides[4 * r + 1],
                         reg_strides[4 * r + 2], reg_strides[4 * r + 3], reg_channels[r], reg_dtype};
        R->dims += reg_channels[r];
    }
    if (R->dims > CHL_MAX_DIM) return PCD_ERR_UNSUPPORTED;
    for (int r = 0; d_hm && r < n_reg; ++r)
        if (!reg_grads[r]) return PCD_ERR_INVALID_ARG;
    return PCD_OK;
}

// the kernels index the maps with 32-bit element counts (below max_elems) and list a frame's objects in LDS
static int chl_check_limits(int batch, int C, int height, int width, int num_max_objs, double max_elems) {
    if ((double)batch * (C > CHL_MAX_DIM ? C : CHL_MAX_DIM) * height * width >= max_elems) return PCD_ERR_UNSUPPORTED;
    if (num_max_objs > CHL_MAX_OBJS) return PCD_ERR_UNSUPPORTED;
    return PCD_OK;
}

}  // namespace
