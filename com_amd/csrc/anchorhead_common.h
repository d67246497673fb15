// What the anchor-head kernels share (anchorhead.hip: AnchorHeadSingle; anchorhead_cur.hip: the COM curriculum form;
// anchorhead_multi.hip: AnchorHeadMulti): table layout, the described anchor and the nearest-BEV pair IoU, the
// prediction-map descriptor, ONE loss core with a compile-time curriculum variant, the ordered second pass and the
// host-side argument checks; the focal element and the ordered pass also serve the point head (roiaware.hip).  Include
// inside the translation unit (everything is file-local).
#pragma once
#include "common.h"

#include <math.h>

#define ANC_KIND_F PCD_ANCHOR_KIND_FLOATS
#define ANC_CLS_F PCD_ANCHOR_CLASS_FLOATS
#define ANC_MAX_KINDS PCD_ANCHOR_MAX_KINDS
#define ANC_MAX_CLASSES PCD_ANCHOR_MAX_CLASSES
#define ANC_MAX_BINS 8

namespace {

enum { K_DX = 0, K_DY, K_DZ, K_ROT, K_ZC, K_SLOT, K_HX, K_HY, K_DIAG };

// kinds -> LDS (every thread of the block calls it; ends with a barrier)
__device__ __forceinline__ void stage_kinds(float *s_kind, const float *kinds, int n_kinds) {
    for (int i = threadIdx.x; i < n_kinds * ANC_KIND_F; i += blockDim.x) s_kind[i] = kinds[i];
    __syncthreads();
}

// ---- the described anchor and the nearest-BEV pair IoU (anchorhead.hip and anchorhead_multi.hip order the anchors
// differently; what an anchor IS, given its kind row and its cell, is the same)
#define ANC_CHUNK 256
#define ANC_BOXF 6      // prepared box: x1, y1, x2, y2, area, class slot (int bits)

struct Anchor {
    float xa, ya, za, dxa, dya, dza, ra, diag;
    float x1, y1, x2, y2, area;
    int slot;
};

// the anchor of kind row `kd` (ANC_KIND_F leading floats) at cell (x, y)
__device__ __forceinline__ Anchor anchor_of_kind(const float *kd, const float *shifts, int x, int y, int W, int H,
                                                 int n_classes) {
    Anchor a;
    a.slot = min(max((int)kd[K_SLOT], 0), n_classes - 1);            // (a table row can never index outside the shifts)
    const float *sh = shifts + (size_t)a.slot * (W + H);
    a.xa = sh[x];
    a.ya = sh[W + y];
    a.dxa = kd[K_DX];
    a.dya = kd[K_DY];
    a.dza = kd[K_DZ];
    a.ra = kd[K_ROT];
    a.za = kd[K_ZC];
    a.diag = kd[K_DIAG];
    // box_utils.py:322-324 with the host's choice of the (dx, dy) | (dy, dx) halves
    a.x1 = a.xa - kd[K_HX];
    a.y1 = a.ya - kd[K_HY];
    a.x2 = a.xa + kd[K_HX];
    a.y2 = a.ya + kd[K_HY];
    a.area = (a.x2 - a.x1) * (a.y2 - a.y1);
    return a;
}

// box_utils.py:301-310 for one pair (0 / x == 0 for the pairs that do not intersect: no division for them)
__device__ __forceinline__ float pair_iou(const Anchor &a, const float *bx) {
    const float x_min = fmaxf(a.x1, bx[0]), x_max = fminf(a.x2, bx[2]);
    const float y_min = fmaxf(a.y1, bx[1]), y_max = fminf(a.y2, bx[3]);
    const float x_len = fmaxf(x_max - x_min, 0.f), y_len = fmaxf(y_max - y_min, 0.f);
    const float inter = x_len * y_len;
    if (!(inter > 0.f)) return 0.f;
    return __fdiv_rn(inter, fmaxf(a.area + bx[4] - inter, 1e-6f));
}

struct AncMaps {            // the three prediction maps (and their gradients): element strides {batch, channel, y, x}
    const void *p[3];
    void *g[3];
    long long s[3][4];
    int dtype;
};

struct AncLossCfg {
    int H, W, A, num_class, num_bins;
    float cls_w, loc_w, dir_w, dir_offset, two_pi, bin_period, inv_batch;
};

// block-wide sum of three floats in a fixed order -> dst[0..3) (thread 0 writes)
__device__ __forceinline__ void block_sum3(float v0, float v1, float v2, float *s_red, float *dst) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        v0 += __shfl_down(v0, d, 64);
        v1 += __shfl_down(v1, d, 64);
        v2 += __shfl_down(v2, d, 64);
    }
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) {
        s_red[w * 3 + 0] = v0;
        s_red[w * 3 + 1] = v1;
        s_red[w * 3 + 2] = v2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) dst[j] = ((s_red[j] + s_red[3 + j]) + s_red[6 + j]) + s_red[9 + j];
    }
}

// The per-anchor curriculum weight of CurriculumSigmoidFocalClassificationLoss.forward (loss_utils.py:236-300) for ONE class
// (num_class == 1: the only shape the reference's get_loss can run).  `sv` is what the state launch saved for this step:
// threshold, variance (1 without NORM), height, elongation, SME gate.
enum { ANC_CUR_OFF = 0, ANC_CUR_SM, ANC_CUR_SMA, ANC_CUR_SIGMOID };
enum { SV_THR = 0, SV_VAR, SV_HEIGHT, SV_ELONG, SV_GATE, SV_FLOATS = 8 };

struct AncCur {
    int mode, oto;
    float smt, pos_norm, neg_norm;
};

__device__ __forceinline__ float anc_cur_weight(const AncCur &q, const float *sv, float p, int group) {
    if (q.mode == ANC_CUR_SM) {                                          // :277-284
        const bool mask = (q.oto ? group > 0 : true) && p <= q.smt;
        return (mask && sv[SV_GATE] != 0.f) ? 0.5f : 1.f;
    }
    if (q.mode == ANC_CUR_SMA) {                                         // :286-289
        const bool mask = group <= 0 && p <= q.smt;
        return (mask && sv[SV_GATE] != 0.f) ? 0.5f : 1.f;
    }
    if (q.mode != ANC_CUR_SIGMOID || (q.oto && !(group > 0))) return 1.f;
    const float thr = sv[SV_THR], h = sv[SV_HEIGHT];                     // :291-300
    const float wgt = h / (1.f + expf(sv[SV_ELONG] * (p - thr) / sv[SV_VAR])) + 1.f - h / 2.f;
    return wgt * (p > thr ? q.pos_norm : q.neg_norm);
}

// One element of SigmoidFocalClassificationLoss (loss_utils.py:41-74), alpha 0.25, gamma 2, for a logit xv and a target t
// in {0, 1}: the unweighted loss (GRAD == false) or its derivative with respect to the logit (GRAD == true).  The anchor
// heads (below) and the point head (roiaware.hip) weight it per anchor / per point.
template <bool GRAD>
__device__ __forceinline__ float focal_el(float xv, float t) {
    const float p = 1.f / (1.f + expf(-xv));
    const float aw = t * 0.25f + (1.f - t) * 0.75f;
    const float pt = t * (1.f - p) + (1.f - t) * p;
    const float bce = fmaxf(xv, 0.f) - xv * t + log1pf(expf(-fabsf(xv)));
    if (!GRAD) return aw * (pt * pt) * bce;
    const float dpt = (1.f - 2.f * t) * p * (1.f - p);
    return aw * (2.f * pt * dpt * bce + pt * pt * (p - t));
}

struct AncNoCur {                   // the plain loss: no extra kernel arguments
    static constexpr bool on = false;
};
struct AncCurArgs {
    static constexpr bool on = true;
    AncCur q;
    const int *groups;              // [B][N] anchor groups (pcd_anchor_cur_groups)
    const float *saved;             // [SV_FLOATS] of this step
};

// One pass over the anchors.  GRAD == false: per-block partial sums of the three losses.  GRAD == true: the gradients
// with respect to the three maps (every element written), scaled by the upstream gradient *grad_out.  CurT == AncCurArgs: the
// positives' anchor weight is multiplied by the (detached) curriculum weight, which thereby scales the focal term, the
// smooth-L1 weights and the direction weights (anchor_head_curriculum.py:159, :221, :241); CurT == AncNoCur compiles to the
// plain loss, instruction for instruction.
template <bool GRAD, class CurT>
__global__ __launch_bounds__(256) void anc_loss_kernel(AncMaps m, AncLossCfg c, const int *labels, const float *reg_targets,
                                                       const int *num_pos, const float *kinds, const float *code_weights,
                                                       const float *grad_out, float *partials, CurT cur) {
    __shared__ float s_kind[ANC_MAX_KINDS * ANC_KIND_F];
    __shared__ float s_red[12];
    const int N = c.H * c.W * c.A;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    stage_kinds(s_kind, kinds, c.A);
    float l_cls = 0.f, l_loc = 0.f, l_dir = 0.f;
    if (n < N) {
        const int cell = n / c.A, k = n - cell * c.A;
        const int y = cell / c.W, x = cell - y * c.W;
        const int label = labels[(size_t)b * N + n];
        const bool pos = label > 0;
        float w = 1.f / fmaxf((float)num_pos[b], 1.f);                 // anchor_head_template.py:118-120, :175-176, :211
        if constexpr (CurT::on) {
            if (pos) {
                const long long off0 = (long long)b * m.s[0][0] + (long long)y * m.s[0][2] + (long long)x * m.s[0][3] +
                                       (long long)(k * c.num_class) * m.s[0][1];
                const float p0 = 1.f / (1.f + expf(-load_el(m.p[0], m.dtype, off0)));
                w *= anc_cur_weight(cur.q, cur.saved, p0, cur.groups[(size_t)b * N + n]);
            }
        }
        float up = 0.f;
        if (GRAD) up = grad_out[0] * c.inv_batch * w;
        long long base[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) base[q] = (long long)b * m.s[q][0] + (long long)y * m.s[q][2] + (long long)x * m.s[q][3];
        // ---- classification: sigmoid focal loss (loss_utils.py:41-74), alpha 0.25, gamma 2
        const int tcls = pos ? (c.num_class == 1 ? 0 : label - 1) : -1;   // :114-116 class agnostic
        for (int j = 0; j < c.num_class; ++j) {
            const long long off = base[0] + (long long)(k * c.num_class + j) * m.s[0][1];
            if (label < 0) {
                if (GRAD) store_el(m.g[0], m.dtype, off, 0.f);
                continue;
            }
            const float xv = load_el(m.p[0], m.dtype, off);
            const float t = (j == tcls) ? 1.f : 0.f;
            if (!GRAD) l_cls += focal_el<false>(xv, t) * w;
            else store_el(m.g[0], m.dtype, off, focal_el<true>(xv, t) * up * c.cls_w);
        }
        // ---- regression: smooth-L1, beta 1/9, with the sin-difference substitution on the heading (:141-148, :192-193)
        const float *tg = reg_targets + ((size_t)b * N + n) * 7;
        const float beta = 1.0f / 9.0f;
        for (int j = 0; j < 7; ++j) {
            const long long off = base[1] + (long long)(k * 7 + j) * m.s[1][1];
            if (!pos) {
                if (GRAD) store_el(m.g[1], m.dtype, off, 0.f);
                continue;
            }
            const float pv = load_el(m.p[1], m.dtype, off), tv = tg[j], cw = code_weights[j];
            float in = pv, ta = tv, din = 1.f;
            if (j == 6) {
                const float sp = sinf(pv), cp = cosf(pv), sn = sinf(tv), cs = cosf(tv);
                in = sp * cs;
                ta = cp * sn;
                din = cp * cs + sp * sn;                                  // d/dp (sin p cos t - cos p sin t)
            }
            const bool nan_t = ta != ta;                                 // loss_utils.py:385: nan targets are ignored
            const float diff = nan_t ? 0.f : (in - ta) * cw;
            const float ad = fabsf(diff);
            if (!GRAD) {
                l_loc += (ad < beta ? 0.5f * (ad * ad) / beta : ad - 0.5f * beta) * w;
            } else {
                const float dl = ad < beta ? diff / beta : (diff > 0.f ? 1.f : -1.f);
                store_el(m.g[1], m.dtype, off, nan_t ? 0.f : dl * din * cw * up * c.loc_w);
            }
        }
        // ---- direction: cross entropy on the heading bin (:150-164, :202-216; loss_utils.py:452-469)
        if (m.p[2]) {
            const int nb = c.num_bins;
            if (!pos) {
                if (GRAD)
                    for (int j = 0; j < nb; ++j) store_el(m.g[2], m.dtype, base[2] + (long long)(k * nb + j) * m.s[2][1], 0.f);
            } else {
                const float rot_gt = tg[6] + s_kind[k * ANC_KIND_F + K_ROT];
                const float v = rot_gt - c.dir_offset;
                const float off_rot = v - floorf(__fdiv_rn(v, c.two_pi) + 0.f) * c.two_pi;
                int bin = (int)floorf(__fdiv_rn(off_rot, c.bin_period));
                bin = bin < 0 ? 0 : (bin > nb - 1 ? nb - 1 : bin);
                float lg[ANC_MAX_BINS];
                float mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < ANC_MAX_BINS; ++j)
                    if (j < nb) {
                        lg[j] = load_el(m.p[2], m.dtype, base[2] + (long long)(k * nb + j) * m.s[2][1]);
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
                            store_el(m.g[2], m.dtype, base[2] + (long long)(k * nb + j) * m.s[2][1],
                                  (expf(lg[j] - lse) - (j == bin ? 1.f : 0.f)) * up * c.dir_w);
                }
            }
        }
    }
    if (!GRAD) block_sum3(l_cls, l_loc, l_dir, s_red, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3);
}

// the ordered second pass: one block, thread t sums partials t, t + 256, ... in that order (fp64), then a fixed tree
__global__ __launch_bounds__(256) void anc_loss_finish_kernel(const float *partials, int n_part, AncLossCfg c, float *out) {
    __shared__ double s[3][256];
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_part; i += 256)
        for (int j = 0; j < 3; ++j) a[j] += (double)partials[(size_t)i * 3 + j];
    for (int j = 0; j < 3; ++j) s[j][threadIdx.x] = a[j];
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d)
            for (int j = 0; j < 3; ++j) s[j][threadIdx.x] += s[j][threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float lc = (float)(s[0][0] * c.inv_batch) * c.cls_w;
        const float ll = (float)(s[1][0] * c.inv_batch) * c.loc_w;
        const float ld = (float)(s[2][0] * c.inv_batch) * c.dir_w;
        out[0] = lc + (ll + ld);                                         // rpn_loss = cls_loss + (loc_loss + dir_loss)
        out[1] = lc;
        out[2] = ll;
        out[3] = ld;
    }
}

bool fill_maps(AncMaps &m, const void *cls, const void *box, const void *dir, void *d_cls, void *d_box, void *d_dir, int dtype,
               const long long *strides_host) {
    if (!cls || !box || !strides_host || (dtype != PCD_F32 && dtype != PCD_BF16)) return false;
    m.p[0] = cls;
    m.p[1] = box;
    m.p[2] = dir;
    m.g[0] = d_cls;
    m.g[1] = d_box;
    m.g[2] = d_dir;
    for (int q = 0; q < 3; ++q)
        for (int j = 0; j < 4; ++j) m.s[q][j] = strides_host[q * 4 + j];
    m.dtype = dtype;
    return true;
}

bool shape_ok(int batch, int height, int width, int n_kinds) {
    if (batch < 1 || height < 1 || width < 1 || n_kinds < 1 || n_kinds > ANC_MAX_KINDS) return false;
    if (batch > 65535) return false;
    return (long long)batch * height * width * n_kinds * 7 < (1ll << 31);
}

bool loss_cfg(AncLossCfg &c, int batch, int height, int width, int n_kinds, int num_class, int num_dir_bins, bool has_dir,
              float cls_weight, float loc_weight, float dir_weight, float dir_offset) {
    if (!shape_ok(batch, height, width, n_kinds) || num_class < 1 || num_class > PCD_ANCHOR_MAX_CLASSES) return false;
    if (has_dir && (num_dir_bins < 1 || num_dir_bins > ANC_MAX_BINS)) return false;
    c.H = height;
    c.W = width;
    c.A = n_kinds;
    c.num_class = num_class;
    c.num_bins = has_dir ? num_dir_bins : 1;
    c.cls_w = cls_weight;
    c.loc_w = loc_weight;
    c.dir_w = dir_weight;
    c.dir_offset = dir_offset;
    c.two_pi = (float)(2.0 * M_PI);
    c.bin_period = (float)(2.0 * M_PI / (double)c.num_bins);
    c.inv_batch = 1.0f / (float)batch;
    return true;
}

}  // namespace
