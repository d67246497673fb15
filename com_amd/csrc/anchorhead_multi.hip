// AnchorHeadMulti on the device (gfx950): target assignment, fused loss, box decoding for per-head prediction maps.
// C ABI: include/pcd_ops.h (f3m).
//
//   pcd_anchor_multi_assign_targets  axis_aligned_target_assigner.py:36-210 with use_multihead (:68-69, :92-101) +
//                                    box_coder_utils.py:13-43 in full (any code size, sin/cos heading)
//   pcd_anchor_multi_loss_forward /  pcdet/models/dense_heads/anchor_head_multi.py:245-373 with loss_utils.py:10-74
//   pcd_anchor_multi_loss_backward   (sigmoid focal), :338-441 (weighted smooth-L1 | weighted L1), :444-469 (cross entropy)
//   pcd_anchor_multi_decode          anchor_head_template.py:229-276 with use_multihead + box_coder_utils.py:45-77
//
// The anchor order is the multi head's: anchor n = (g * H + y) * W + x, g the global kind; head h owns a contiguous run
// of kinds.  A block of 256 consecutive anchors straddles kinds -- and heads -- whenever H * W is no multiple of 256, so
// every thread resolves its own head from a kind -> head table in LDS, beside a copy of the head descriptors; one launch
// covers all heads.  The assignment is the single head's (anchorhead.hip): same three launches, same pair IoU
// (anchorhead_common.h), integer atomic max, `== maximum` forcing, lowest index on ties; no [N, M] matrix, no cap on M.
// Compiled with -ffp-contract=off like anchorhead.hip, for the same reason.
#include "anchorhead_common.h"

#define AM_KIND_F PCD_ANCHOR_MULTI_KIND_FLOATS
#define AM_MAX_HEADS PCD_ANCHOR_MULTI_MAX_HEADS
#define AM_MAX_CODE PCD_ANCHOR_MULTI_MAX_CODE

namespace {

enum { K_COS = 10, K_SIN = 11 };

struct AmHeads {                    // the head descriptors as a kernel argument
    PcdAnchorMultiHead h[AM_MAX_HEADS];
    int n;
};

struct AmGeom {                     // anchor n of a frame -> global kind and cell
    int g, y, x;
};

__device__ __forceinline__ AmGeom am_geom(int n, int H, int W) {
    AmGeom q;
    const int HW = H * W;
    q.g = n / HW;
    const int cell = n - q.g * HW;
    q.y = cell / W;
    q.x = cell - q.y * W;
    return q;
}

// kinds -> LDS (every thread of the block calls it; ends with a barrier)
__device__ __forceinline__ void am_stage_kinds(float *s_kind, const float *kinds, int n_kinds) {
    for (int i = threadIdx.x; i < n_kinds * AM_KIND_F; i += blockDim.x) s_kind[i] = kinds[i];
    __syncthreads();
}

// head descriptors + the kind -> head table -> LDS (every thread of the block calls it; ends with a barrier).  The host
// checked that the heads tile [0, n_kinds) in order, so every entry of s_head_of_kind below n_kinds is written.
__device__ __forceinline__ void am_stage_heads(PcdAnchorMultiHead *s_head, int *s_head_of_kind, const AmHeads &hd) {
    for (int h = threadIdx.x; h < hd.n; h += blockDim.x) {
        s_head[h] = hd.h[h];
        for (int k = 0; k < hd.h[h].n_kinds; ++k) s_head_of_kind[hd.h[h].kind0 + k] = h;
    }
    __syncthreads();
}

// ---- launch 1: boxes -> aligned BEV boxes, class slots; clears the per-box maxima and the positive counts
//      (anchorhead.hip's anc_prep_kernel for rows of `row` floats with the class id last)
__global__ __launch_bounds__(256) void am_prep_kernel(const float *gt, int B, int M, int row, const float *classes,
                                                      int n_classes, float *pb, u32 *box_max, int *num_pos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) num_pos[i] = 0;
    if (i >= B * M) return;
    const float *g = gt + (size_t)i * row;
    const float pi = 3.14159265358979323846f;                          // np.pi as fp32
    const float r = g[6];
    const float ang = fabsf(r - floorf(__fdiv_rn(r, pi) + 0.5f) * pi);   // common_utils.limit_period(r, 0.5, pi).abs()
    const bool keep = ang < 0.78539816339744830962f;                   // < np.pi / 4
    const float cx = keep ? g[3] : g[4], cy = keep ? g[4] : g[3];
    const float x1 = g[0] - cx / 2.f, y1 = g[1] - cy / 2.f, x2 = g[0] + cx / 2.f, y2 = g[1] + cy / 2.f;
    const int cls = (int)g[row - 1];
    int slot = -1;
    if (cls > 0)
        for (int c = 0; c < n_classes; ++c)
            if ((int)classes[c * ANC_CLS_F + 2] == cls) slot = c;
    float *o = pb + (size_t)i * ANC_BOXF;
    o[0] = x1;
    o[1] = y1;
    o[2] = x2;
    o[3] = y2;
    o[4] = (x2 - x1) * (y2 - y1);
    o[5] = __int_as_float(slot);
    box_max[i] = 0u;
}

struct AmAssignCfg {
    int H, W, G, n_classes, M, row, code, sincos;
};

// ---- launches 2 and 3.  FINAL == false: per-box maximum.  FINAL == true: labels, targets, weights, positive counts.
template <bool FINAL>
__global__ __launch_bounds__(256) void am_assign_kernel(AmAssignCfg c, const float *gt, const float *pb, u32 *box_max,
                                                        const float *kinds, const float *classes, const float *shifts,
                                                        int *labels, float *reg_targets, float *reg_weights, int *gt_index,
                                                        int *num_pos) {
    __shared__ float s_kind[ANC_MAX_KINDS * AM_KIND_F];
    __shared__ float s_box[ANC_CHUNK * ANC_BOXF];
    __shared__ int s_cnt[4];
    const int N = c.H * c.W * c.G, M = c.M;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool valid = n < N;
    am_stage_kinds(s_kind, kinds, c.G);
    const AmGeom q = am_geom(valid ? n : 0, c.H, c.W);
    const float *kd = s_kind + q.g * AM_KIND_F;
    const Anchor a = anchor_of_kind(kd, shifts, q.x, q.y, c.W, c.H, c.n_classes);
    float best = 0.f;
    int arg = -1;
    bool forced = false;
    for (int m0 = 0; m0 < M; m0 += ANC_CHUNK) {
        const int cnt = min(ANC_CHUNK, M - m0);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * ANC_BOXF; i += 256) s_box[i] = pb[((size_t)b * M + m0) * ANC_BOXF + i];
        __syncthreads();
        if (!valid) continue;
        for (int j = 0; j < cnt; ++j) {
            const float *bx = s_box + j * ANC_BOXF;
            if (__float_as_int(bx[5]) != a.slot) continue;
            const float iou = pair_iou(a, bx);
            if (!(iou > 0.f)) continue;
            if (!FINAL) {
                atomicMax(box_max + (size_t)b * M + m0 + j, __float_as_uint(iou));
            } else {
                if (iou > best) {                                        // lowest index on ties (argmax(dim=1))
                    best = iou;
                    arg = m0 + j;
                }
                if (__float_as_uint(iou) == box_max[(size_t)b * M + m0 + j]) forced = true;   // :155
            }
        }
    }
    if (!FINAL) return;
    int positive = 0;
    if (valid) {
        const float *cl = classes + a.slot * ANC_CLS_F;
        const size_t o = (size_t)b * N + n;
        float t[AM_MAX_CODE];
#pragma unroll
        for (int j = 0; j < AM_MAX_CODE; ++j) t[j] = 0.f;
        int label;
        if (forced || (arg >= 0 && best >= cl[0])) {                     // :157, :162, :188
            label = (int)cl[2];
            positive = label > 0;
        } else {
            label = best < cl[1] ? 0 : -1;                               // :164, :187
        }
        if (positive) {                                                  // box_coder_utils.py:22-43
            const float *g = gt + ((size_t)b * M + arg) * c.row;
            const float dxa = fmaxf(a.dxa, 1e-5f), dya = fmaxf(a.dya, 1e-5f), dza = fmaxf(a.dza, 1e-5f);
            const float dxg = fmaxf(g[3], 1e-5f), dyg = fmaxf(g[4], 1e-5f), dzg = fmaxf(g[5], 1e-5f);
            t[0] = __fdiv_rn(g[0] - a.xa, a.diag);
            t[1] = __fdiv_rn(g[1] - a.ya, a.diag);
            t[2] = __fdiv_rn(g[2] - a.za, dza);
            t[3] = logf(__fdiv_rn(dxg, dxa));
            t[4] = logf(__fdiv_rn(dyg, dya));
            t[5] = logf(__fdiv_rn(dzg, dza));
            // the extra columns between the heading and the class id (:42; the anchor's are zeros)
            const bool extras = c.row > 8;
            const float e0 = extras ? g[7] - 0.f : 0.f, e1 = extras ? g[8] - 0.f : 0.f;
            if (c.sincos) {                                              // :35-38
                t[6] = cosf(g[6]) - kd[K_COS];
                t[7] = sinf(g[6]) - kd[K_SIN];
                t[8] = e0;
                t[9] = e1;
            } else {
                t[6] = g[6] - a.ra;
                t[7] = e0;
                t[8] = e1;
            }
        }
        labels[o] = label;
#pragma unroll
        for (int j = 0; j < AM_MAX_CODE; ++j)
            if (j < c.code) reg_targets[o * c.code + j] = t[j];
        reg_weights[o] = positive ? 1.f : 0.f;
        if (gt_index) gt_index[o] = positive ? arg : -1;
    }
    // positives of this block -> num_pos[b] (integer atomics: order independent)
    const int wave_cnt = __popcll(__ballot(positive != 0));
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = wave_cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int k = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (k) atomicAdd(num_pos + b, k);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct AmLossCfg {
    int H, W, G, num_class, code, l1, num_bins, has_dir, dtype;
    float pos_w, neg_w, cls_w, loc_w, dir_w, dir_offset, two_pi, bin_period, inv_batch;
};

// One pass over the anchors of all heads.  GRAD == false: per-block partial sums of the three losses.  GRAD == true: the
// gradients with respect to every head's maps (every element written), scaled by the upstream gradient *grad_out.
template <bool GRAD>
__global__ __launch_bounds__(256) void am_loss_kernel(AmHeads hd, AmLossCfg c, const int *labels, const float *reg_targets,
                                                      const int *num_pos, const float *kinds, const float *code_weights,
                                                      const float *grad_out, float *partials) {
    __shared__ float s_kind[ANC_MAX_KINDS * AM_KIND_F];
    __shared__ PcdAnchorMultiHead s_head[AM_MAX_HEADS];
    __shared__ int s_head_of_kind[ANC_MAX_KINDS];
    __shared__ float s_red[12];
    const int N = c.H * c.W * c.G;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    am_stage_heads(s_head, s_head_of_kind, hd);
    am_stage_kinds(s_kind, kinds, c.G);
    float l_cls = 0.f, l_loc = 0.f, l_dir = 0.f;
    if (n < N) {
        const AmGeom q = am_geom(n, c.H, c.W);
        const PcdAnchorMultiHead &hh = s_head[s_head_of_kind[q.g]];
        const int k = q.g - hh.kind0;                                    // the anchor's kind inside its head
        const int nc = hh.num_class;
        const int label = labels[(size_t)b * N + n];
        const bool pos = label > 0;
        const float norm = fmaxf((float)num_pos[b], 1.f);              // anchor_head_multi.py:269-272, :311-312, :363
        const float w = 1.f / norm;                                      // regression and direction weight
        const float wc = __fdiv_rn(pos ? c.pos_w : c.neg_w, norm);       // :261-263 (label < 0: no term at all)
        float up = 0.f, upc = 0.f;
        if (GRAD) {
            up = grad_out[0] * c.inv_batch * w;
            upc = grad_out[0] * c.inv_batch * wc;
        }
        long long base[3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
            base[m] = (long long)b * hh.strides[m][0] + (long long)q.y * hh.strides[m][2] + (long long)q.x * hh.strides[m][3];
        // ---- classification: sigmoid focal loss on the head's class slice of the global one-hot (:274-292)
        const int tcls = pos ? (c.num_class == 1 ? 0 : label - 1) - hh.class0 : -1;   // :266-268 class agnostic
        for (int j = 0; j < nc; ++j) {
            const long long off = base[0] + (long long)(k * nc + j) * hh.strides[0][1];
            if (label < 0) {
                if (GRAD) store_el(hh.grad[0], c.dtype, off, 0.f);
                continue;
            }
            const float xv = load_el(hh.map[0], c.dtype, off);
            const float t = (j == tcls) ? 1.f : 0.f;
            if (!GRAD) l_cls += focal_el<false>(xv, t) * wc;
            else store_el(hh.grad[0], c.dtype, off, focal_el<true>(xv, t) * upc * c.cls_w);
        }
        // ---- regression: smooth-L1 (beta 1/9) | L1 on the codes; with direction maps the sin-difference substitution on
        //      code 6 (:341-345)
        const float *tg = reg_targets + ((size_t)b * N + n) * c.code;
        const float beta = 1.0f / 9.0f;
        for (int j = 0; j < c.code; ++j) {
            const long long off = base[1] + (long long)(k * c.code + j) * hh.strides[1][1];
            if (!pos) {
                if (GRAD) store_el(hh.grad[1], c.dtype, off, 0.f);
                continue;
            }
            const float pv = load_el(hh.map[1], c.dtype, off), tv = tg[j], cw = code_weights[j];
            float in = pv, ta = tv, din = 1.f;
            if (c.has_dir && j == 6) {
                const float sp = sinf(pv), cp = cosf(pv), sn = sinf(tv), cs = cosf(tv);
                in = sp * cs;
                ta = cp * sn;
                din = cp * cs + sp * sn;                                  // d/dp (sin p cos t - cos p sin t)
            }
            const bool nan_t = ta != ta;                                 // loss_utils.py:385, :427: nan targets are ignored
            const float diff = nan_t ? 0.f : (in - ta) * cw;
            const float ad = fabsf(diff);
            if (!GRAD) {
                const float el = c.l1 ? ad : (ad < beta ? 0.5f * (ad * ad) / beta : ad - 0.5f * beta);
                l_loc += el * w;
            } else {
                const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                const float dl = (!c.l1 && ad < beta) ? diff / beta : sgn;
                store_el(hh.grad[1], c.dtype, off, nan_t ? 0.f : dl * din * cw * up * c.loc_w);
            }
        }
        // ---- direction: cross entropy on the heading bin (:352-371; anchor_head_template.py:150-164)
        if (c.has_dir) {
            const int nb = c.num_bins;
            if (!pos) {
                if (GRAD)
                    for (int j = 0; j < nb; ++j)
                        store_el(hh.grad[2], c.dtype, base[2] + (long long)(k * nb + j) * hh.strides[2][1], 0.f);
            } else {
                const float rot_gt = tg[6] + s_kind[q.g * AM_KIND_F + K_ROT];
                const float v = rot_gt - c.dir_offset;
                const float off_rot = v - floorf(__fdiv_rn(v, c.two_pi) + 0.f) * c.two_pi;
                int bin = (int)floorf(__fdiv_rn(off_rot, c.bin_period));
                bin = bin < 0 ? 0 : (bin > nb - 1 ? nb - 1 : bin);
                float lg[ANC_MAX_BINS];
                float mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < ANC_MAX_BINS; ++j)
                    if (j < nb) {
                        lg[j] = load_el(hh.map[2], c.dtype, base[2] + (long long)(k * nb + j) * hh.strides[2][1]);
                        mx = fmaxf(mx, lg[j]);
                    }
                float se = 0.f, lb = 0.f;
#pragma unroll
                for (int j = 0; j < ANC_MAX_BINS; ++j)
                    if (j < nb) {
                        se += expf(lg[j] - mx);
                        if (j == bin) lb = lg[j];
                    }
                const float lse = mx + logf(se);
                if (!GRAD) {
                    l_dir = (lse - lb) * w;
                } else {
#pragma unroll
                    for (int j = 0; j < ANC_MAX_BINS; ++j)
                        if (j < nb)
                            store_el(hh.grad[2], c.dtype, base[2] + (long long)(k * nb + j) * hh.strides[2][1],
                                     (expf(lg[j] - lse) - (j == bin ? 1.f : 0.f)) * up * c.dir_w);
                }
            }
        }
    }
    if (!GRAD) block_sum3(l_cls, l_loc, l_dir, s_red, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3);
}

// ---------------------------------------------------------------------------------------------------------------------
struct AmDecodeCfg {
    int H, W, G, n_classes, code, sincos, num_bins, has_dir, dtype;
    float dir_offset, dir_limit_offset, period;
};

struct AmClsOut {
    float *p[AM_MAX_HEADS];
};

__global__ __launch_bounds__(256) void am_decode_kernel(AmHeads hd, AmDecodeCfg c, const float *kinds, const float *shifts,
                                                        float *box_out, AmClsOut cls_out) {
    __shared__ float s_kind[ANC_MAX_KINDS * AM_KIND_F];
    __shared__ PcdAnchorMultiHead s_head[AM_MAX_HEADS];
    __shared__ float *s_cls_out[AM_MAX_HEADS];
    __shared__ int s_head_of_kind[ANC_MAX_KINDS];
    const int HW = c.H * c.W, N = HW * c.G;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    for (int h = threadIdx.x; h < hd.n; h += blockDim.x) s_cls_out[h] = cls_out.p[h];
    am_stage_heads(s_head, s_head_of_kind, hd);
    am_stage_kinds(s_kind, kinds, c.G);
    if (n >= N) return;
    const AmGeom q = am_geom(n, c.H, c.W);
    const int h = s_head_of_kind[q.g];
    const PcdAnchorMultiHead &hh = s_head[h];
    const float *kd = s_kind + q.g * AM_KIND_F;
    const Anchor a = anchor_of_kind(kd, shifts, q.x, q.y, c.W, c.H, c.n_classes);
    const int k = q.g - hh.kind0, nc = hh.num_class;
    long long base[3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
        base[m] = (long long)b * hh.strides[m][0] + (long long)q.y * hh.strides[m][2] + (long long)q.x * hh.strides[m][3];
    // the head's logits [B][N_h][C_h]
    const size_t n_h = (size_t)hh.n_kinds * HW, local = (size_t)n - (size_t)hh.kind0 * HW;
    float *co = s_cls_out[h] + ((size_t)b * n_h + local) * nc;
    for (int j = 0; j < nc; ++j) co[j] = load_el(hh.map[0], c.dtype, base[0] + (long long)(k * nc + j) * hh.strides[0][1]);
    float t[AM_MAX_CODE];
#pragma unroll
    for (int j = 0; j < AM_MAX_CODE; ++j)
        t[j] = j < c.code ? load_el(hh.map[1], c.dtype, base[1] + (long long)(k * c.code + j) * hh.strides[1][1]) : 0.f;
    float r[9];                                                          // box_coder_utils.py:54-77
    r[0] = t[0] * a.diag + a.xa;
    r[1] = t[1] * a.diag + a.ya;
    r[2] = t[2] * a.dza + a.za;
    r[3] = expf(t[3]) * a.dxa;
    r[4] = expf(t[4]) * a.dya;
    r[5] = expf(t[5]) * a.dza;
    if (c.sincos) r[6] = atan2f(t[7] + kd[K_SIN], t[6] + kd[K_COS]);     // :69-72
    else r[6] = t[6] + a.ra;
    r[7] = (c.sincos ? t[8] : t[7]) + 0.f;                               // :76, the anchor's extra columns are zeros
    r[8] = (c.sincos ? t[9] : t[8]) + 0.f;
    if (c.has_dir) {                                                     // anchor_head_template.py:258-269
        int lab = 0;
        float mx = load_el(hh.map[2], c.dtype, base[2] + (long long)(k * c.num_bins) * hh.strides[2][1]);
        for (int j = 1; j < c.num_bins; ++j) {
            const float v = load_el(hh.map[2], c.dtype, base[2] + (long long)(k * c.num_bins + j) * hh.strides[2][1]);
            if (v > mx) {
                mx = v;
                lab = j;
            }
        }
        const float v = r[6] - c.dir_offset;
        const float dir_rot = v - floorf(__fdiv_rn(v, c.period) + c.dir_limit_offset) * c.period;
        r[6] = (dir_rot + c.dir_offset) + c.period * (float)lab;
    }
    const int ow = c.code - c.sincos;
    float *bo = box_out + ((size_t)b * N + n) * ow;
#pragma unroll
    for (int j = 0; j < 9; ++j)
        if (j < ow) bo[j] = r[j];
}

// ---- host-side checks --------------------------------------------------------------------------------------------
bool am_code_ok(int code, int sincos) {
    const int code_gt = code - sincos;
    return (sincos == 0 || sincos == 1) && (code_gt == 7 || code_gt == 9);
}

bool am_shape_ok(int batch, int height, int width, int n_kinds, int code) {
    if (!shape_ok(batch, height, width, n_kinds)) return false;
    return (long long)batch * height * width * n_kinds * code < (1ll << 31);
}

// heads -> the kernel argument; false unless they tile the kinds [0, n_kinds) and the classes [0, num_class) in order and
// agree on the direction maps.  need_grad: the three (two) gradient pointers must be there.
bool am_fill_heads(AmHeads &hd, const PcdAnchorMultiHead *heads, int n_heads, int n_kinds, int num_class, bool need_grad,
                   bool &has_dir) {
    if (!heads || n_heads < 1 || n_heads > AM_MAX_HEADS) return false;
    int kind = 0, cls = 0;
    has_dir = heads[0].map[2] != nullptr;
    for (int h = 0; h < n_heads; ++h) {
        const PcdAnchorMultiHead &s = heads[h];
        if (!s.map[0] || !s.map[1] || (s.map[2] != nullptr) != has_dir) return false;
        if (need_grad && (!s.grad[0] || !s.grad[1] || (has_dir && !s.grad[2]))) return false;
        if (s.kind0 != kind || s.n_kinds < 1 || s.class0 != cls || s.num_class < 1) return false;
        kind += s.n_kinds;
        cls += s.num_class;
        hd.h[h] = s;
        if (!has_dir) {                                                  // (no row of the table is left unset)
            hd.h[h].grad[2] = nullptr;
            for (int j = 0; j < 4; ++j) hd.h[h].strides[2][j] = 0;
        }
    }
    for (int h = n_heads; h < AM_MAX_HEADS; ++h) hd.h[h] = PcdAnchorMultiHead{};
    hd.n = n_heads;
    return kind == n_kinds && cls == num_class;
}

bool am_loss_cfg(AmLossCfg &c, int dtype, int batch, int height, int width, int n_kinds, int num_class, int code, int reg_l1,
                 int num_dir_bins, bool has_dir, float pos_w, float neg_w, float cls_weight, float loc_weight, float dir_weight,
                 float dir_offset) {
    if (dtype != PCD_F32 && dtype != PCD_BF16) return false;
    if (code < 7 || code > AM_MAX_CODE || !am_shape_ok(batch, height, width, n_kinds, code)) return false;
    if (num_class < 1 || num_class > PCD_ANCHOR_MAX_CLASSES || (reg_l1 != 0 && reg_l1 != 1)) return false;
    if (has_dir && (num_dir_bins < 1 || num_dir_bins > ANC_MAX_BINS)) return false;
    c.H = height;
    c.W = width;
    c.G = n_kinds;
    c.num_class = num_class;
    c.code = code;
    c.l1 = reg_l1;
    c.num_bins = has_dir ? num_dir_bins : 1;
    c.has_dir = has_dir ? 1 : 0;
    c.dtype = dtype;
    c.pos_w = pos_w;
    c.neg_w = neg_w;
    c.cls_w = cls_weight;
    c.loc_w = loc_weight;
    c.dir_w = has_dir ? dir_weight : 0.f;
    c.dir_offset = dir_offset;
    c.two_pi = (float)(2.0 * M_PI);
    c.bin_period = (float)(2.0 * M_PI / (double)c.num_bins);
    c.inv_batch = 1.0f / (float)batch;
    return true;
}

}  // namespace

extern "C" size_t pcd_anchor_multi_assign_workspace_bytes(int batch, int n_boxes) {
    if (batch < 1 || n_boxes < 0) return 0;
    const size_t bm = (size_t)batch * (size_t)(n_boxes > 0 ? n_boxes : 1);
    return ws_piece(bm * ANC_BOXF, sizeof(float)) + ws_piece(bm, sizeof(u32));
}

extern "C" int pcd_anchor_multi_assign_targets(const float *gt_boxes, int batch, int n_boxes, int code_gt, int sincos,
                                               const float *kinds, int n_kinds, const float *classes, int n_classes,
                                               const float *shifts, int height, int width, int *box_cls_labels,
                                               float *box_reg_targets, float *reg_weights, int *gt_index, int *num_pos,
                                               void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    if (!kinds || !classes || !shifts || !box_cls_labels || !box_reg_targets || !reg_weights || !num_pos || n_boxes < 0 ||
        (n_boxes > 0 && !gt_boxes))
        return PCD_ERR_INVALID_ARG;
    if (!am_code_ok(code_gt + sincos, sincos) || !am_shape_ok(batch, height, width, n_kinds, code_gt + sincos) ||
        n_classes < 1 || n_classes > ANC_MAX_CLASSES || (long long)batch * n_boxes >= (1ll << 27))
        return PCD_ERR_UNSUPPORTED;
    WsCarver ws(workspace, workspace_bytes);
    const size_t bm = (size_t)batch * (size_t)(n_boxes > 0 ? n_boxes : 1);
    float *pb = ws.take<float>(bm * ANC_BOXF);
    u32 *box_max = ws.take<u32>(bm);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    AmAssignCfg c;
    c.H = height;
    c.W = width;
    c.G = n_kinds;
    c.n_classes = n_classes;
    c.M = n_boxes;
    c.row = code_gt + 1;
    c.code = code_gt + sincos;
    c.sincos = sincos;
    const int N = height * width * n_kinds;
    const int prep_n = batch * n_boxes > batch ? batch * n_boxes : batch;
    am_prep_kernel<<<pcd_div_up(prep_n, 256), 256, 0, st>>>(gt_boxes, batch, n_boxes, c.row, classes, n_classes, pb, box_max,
                                                            num_pos);
    dim3 grid(pcd_div_up(N, 256), batch);
    am_assign_kernel<false><<<grid, 256, 0, st>>>(c, gt_boxes, pb, box_max, kinds, classes, shifts, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr);
    am_assign_kernel<true><<<grid, 256, 0, st>>>(c, gt_boxes, pb, box_max, kinds, classes, shifts, box_cls_labels,
                                                 box_reg_targets, reg_weights, gt_index, num_pos);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" size_t pcd_anchor_multi_loss_workspace_bytes(int batch, int height, int width, int n_kinds) {
    if (!shape_ok(batch, height, width, n_kinds)) return 0;
    return ws_piece((size_t)batch * pcd_div_up(height * width * n_kinds, 256) * 3, sizeof(float));
}

extern "C" int pcd_anchor_multi_loss_forward(const PcdAnchorMultiHead *heads, int n_heads, int dtype, const int *box_cls_labels,
                                             const float *box_reg_targets, const int *num_pos, int batch, int height, int width,
                                             int n_kinds, int num_class, int code, int reg_l1, int num_dir_bins,
                                             const float *kinds, const float *code_weights, float pos_cls_weight,
                                             float neg_cls_weight, float cls_weight, float loc_weight, float dir_weight,
                                             float dir_offset, float *out, void *workspace, size_t workspace_bytes,
                                             void *stream) {
    PCD_ENTER();
    AmHeads hd;
    AmLossCfg c;
    bool has_dir = false;
    if (!box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights || !out) return PCD_ERR_INVALID_ARG;
    if (!am_loss_cfg(c, dtype, batch, height, width, n_kinds, num_class, code, reg_l1, num_dir_bins,
                     heads && heads[0].map[2] != nullptr, pos_cls_weight, neg_cls_weight, cls_weight, loc_weight, dir_weight,
                     dir_offset))
        return PCD_ERR_UNSUPPORTED;
    if (!am_fill_heads(hd, heads, n_heads, n_kinds, num_class, false, has_dir)) return PCD_ERR_INVALID_ARG;
    WsCarver ws(workspace, workspace_bytes);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    float *partials = ws.take<float>((size_t)grid.x * grid.y * 3);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    AncLossCfg fin = {};                                                 // what the ordered second pass reads
    fin.cls_w = c.cls_w;
    fin.loc_w = c.loc_w;
    fin.dir_w = c.dir_w;
    fin.inv_batch = c.inv_batch;
    hipStream_t st = (hipStream_t)stream;
    am_loss_kernel<false><<<grid, 256, 0, st>>>(hd, c, box_cls_labels, box_reg_targets, num_pos, kinds, code_weights, nullptr,
                                                partials);
    anc_loss_finish_kernel<<<1, 256, 0, st>>>(partials, (int)(grid.x * grid.y), fin, out);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_multi_loss_backward(const PcdAnchorMultiHead *heads, int n_heads, int dtype, const int *box_cls_labels,
                                              const float *box_reg_targets, const int *num_pos, int batch, int height,
                                              int width, int n_kinds, int num_class, int code, int reg_l1, int num_dir_bins,
                                              const float *kinds, const float *code_weights, float pos_cls_weight,
                                              float neg_cls_weight, float cls_weight, float loc_weight, float dir_weight,
                                              float dir_offset, const float *grad_out, void *stream) {
    PCD_ENTER();
    AmHeads hd;
    AmLossCfg c;
    bool has_dir = false;
    if (!box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights || !grad_out) return PCD_ERR_INVALID_ARG;
    if (!am_loss_cfg(c, dtype, batch, height, width, n_kinds, num_class, code, reg_l1, num_dir_bins,
                     heads && heads[0].map[2] != nullptr, pos_cls_weight, neg_cls_weight, cls_weight, loc_weight, dir_weight,
                     dir_offset))
        return PCD_ERR_UNSUPPORTED;
    if (!am_fill_heads(hd, heads, n_heads, n_kinds, num_class, true, has_dir)) return PCD_ERR_INVALID_ARG;
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    am_loss_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(hd, c, box_cls_labels, box_reg_targets, num_pos, kinds,
                                                                code_weights, grad_out, nullptr);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_multi_decode(const PcdAnchorMultiHead *heads, int n_heads, int dtype, int batch, int height, int width,
                                       int n_kinds, int n_classes, int code, int sincos, int num_dir_bins, const float *kinds,
                                       const float *shifts, float dir_offset, float dir_limit_offset, float *batch_box_preds,
                                       float *const *cls_out_host, void *stream) {
    PCD_ENTER();
    AmHeads hd;
    bool has_dir = false;
    if (!kinds || !shifts || !batch_box_preds || !cls_out_host || (dtype != PCD_F32 && dtype != PCD_BF16))
        return PCD_ERR_INVALID_ARG;
    if (!am_code_ok(code, sincos) || !am_shape_ok(batch, height, width, n_kinds, code) || n_classes < 1 ||
        n_classes > ANC_MAX_CLASSES)
        return PCD_ERR_UNSUPPORTED;
    if (!heads || n_heads < 1 || n_heads > AM_MAX_HEADS) return PCD_ERR_INVALID_ARG;
    int num_class = 0;
    for (int h = 0; h < n_heads; ++h) num_class += heads[h].num_class;
    if (num_class > PCD_ANCHOR_MAX_CLASSES) return PCD_ERR_UNSUPPORTED;
    if (!am_fill_heads(hd, heads, n_heads, n_kinds, num_class, false, has_dir)) return PCD_ERR_INVALID_ARG;
    if (has_dir && (num_dir_bins < 1 || num_dir_bins > ANC_MAX_BINS)) return PCD_ERR_UNSUPPORTED;
    AmClsOut co = {};
    for (int h = 0; h < n_heads; ++h) {
        if (!cls_out_host[h]) return PCD_ERR_INVALID_ARG;
        if ((long long)batch * height * width * heads[h].n_kinds * heads[h].num_class >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
        co.p[h] = cls_out_host[h];
    }
    AmDecodeCfg c;
    c.H = height;
    c.W = width;
    c.G = n_kinds;
    c.n_classes = n_classes;
    c.code = code;
    c.sincos = sincos;
    c.num_bins = has_dir ? num_dir_bins : 1;
    c.has_dir = has_dir ? 1 : 0;
    c.dtype = dtype;
    c.dir_offset = dir_offset;
    c.dir_limit_offset = dir_limit_offset;
    c.period = (float)(2.0 * M_PI / (double)c.num_bins);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    am_decode_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(hd, c, kinds, shifts, batch_box_preds, co);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
