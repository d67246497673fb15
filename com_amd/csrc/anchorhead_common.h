// The core of the anchor heads: ONE box preparation, assignment, loss, decoding and ordered-finish kernel, the host-side
// argument checks, and the two LAYOUTS that are all the heads differ in (anchorhead.hip: AnchorHeadSingle, cell-major;
// anchorhead_cur.hip: its COM curriculum form; anchorhead_multi.hip: AnchorHeadMulti, kind-major).  A layout says how
// anchor n becomes (global kind, y, x), how wide a kind row is, which head descriptor owns a kind and where the logits
// of an anchor go in the decode output; everything else -- the rule of the assignment, the arithmetic of the loss, the
// coder -- exists once.  focal_el and the ordered finish also serve the point heads (pointhead.hip).  Include inside the
// translation unit (everything is file-local).
#pragma once
#include "common.h"

#include <math.h>

#define ANC_CLS_F PCD_ANCHOR_CLASS_FLOATS
#define ANC_MAX_KINDS PCD_ANCHOR_MAX_KINDS
#define ANC_MAX_CLASSES PCD_ANCHOR_MAX_CLASSES
#define ANC_MAX_HEADS PCD_ANCHOR_MULTI_MAX_HEADS
#define ANC_MAX_CODE PCD_ANCHOR_MULTI_MAX_CODE
#define ANC_MAX_BINS 8

namespace {

enum { K_DX = 0, K_DY, K_DZ, K_ROT, K_ZC, K_SLOT, K_HX, K_HY, K_DIAG, K_COS = 10, K_SIN = 11 };   // (10, 11: kind-major rows only)

// `n` floats -> LDS (every thread of the block calls it; ends with a barrier)
__device__ __forceinline__ void stage_kinds(float *s_kind, const float *kinds, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) s_kind[i] = kinds[i];
    __syncthreads();
}

// ---- layouts ----------------------------------------------------------------------------------------------------------
// the descriptor of one head: three maps, their gradients, element strides, kind0 / n_kinds / class0 / num_class
typedef PcdAnchorMultiHead AncHead;

struct AncGeom {                    // anchor n of a frame -> global kind and cell
    int g, y, x;
};

// AnchorHeadSingle: n = (y * W + x) * G + g, the reference's (y, x, class, size, rotation) order; ONE head, held by value in
// the kernel arguments (no LDS, no barrier); logits [B][N][num_class].
struct CellMajor {
    static constexpr int KIND_F = PCD_ANCHOR_KIND_FLOATS;
    struct Shared {};
    AncHead h;
    float *cls_out;
    static __device__ __forceinline__ AncGeom geom(int n, int H, int W, int G) {
        AncGeom q;
        const int cell = n / G;
        q.g = n - cell * G;
        q.y = cell / W;
        q.x = cell - q.y * W;
        return q;
    }
    __device__ __forceinline__ void stage(Shared &) const {}
    __device__ __forceinline__ const AncHead &head(const Shared &, int) const { return h; }
    __device__ __forceinline__ float *logit_row(const Shared &, const AncHead &hh, int b, int n, int HW, int N) const {
        return cls_out + ((size_t)b * N + n) * hh.num_class;
    }
};

// AnchorHeadMulti: n = (g * H + y) * W + x; head h owns a contiguous run of kinds.  A block of 256 consecutive anchors
// straddles kinds -- and heads -- whenever H * W is no multiple of 256, so every thread resolves its own head from a
// kind -> head table in LDS, beside a copy of the descriptors; logits per head [B][N_h][C_h].
struct KindMajor {
    static constexpr int KIND_F = PCD_ANCHOR_MULTI_KIND_FLOATS;
    struct Shared {
        AncHead head[ANC_MAX_HEADS];
        float *cls_out[ANC_MAX_HEADS];
        int head_of_kind[ANC_MAX_KINDS];
    };
    AncHead h[ANC_MAX_HEADS];
    float *cls_out[ANC_MAX_HEADS];
    int n;
    static __device__ __forceinline__ AncGeom geom(int n, int H, int W, int G) {
        AncGeom q;
        const int HW = H * W;
        q.g = n / HW;
        const int cell = n - q.g * HW;
        q.y = cell / W;
        q.x = cell - q.y * W;
        return q;
    }
    // (every thread of the block calls it; ends with a barrier.  The host checked that the heads tile [0, n_kinds) in
    //  order, so every entry of head_of_kind below n_kinds is written.)
    __device__ __forceinline__ void stage(Shared &s) const {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            s.head[i] = h[i];
            s.cls_out[i] = cls_out[i];
            for (int k = 0; k < h[i].n_kinds; ++k) s.head_of_kind[h[i].kind0 + k] = i;
        }
        __syncthreads();
    }
    __device__ __forceinline__ const AncHead &head(const Shared &s, int g) const { return s.head[s.head_of_kind[g]]; }
    __device__ __forceinline__ float *logit_row(const Shared &s, const AncHead &hh, int b, int n, int HW, int N) const {
        const size_t n_h = (size_t)hh.n_kinds * HW, local = (size_t)n - (size_t)hh.kind0 * HW;
        return s.cls_out[&hh - s.head] + ((size_t)b * n_h + local) * hh.num_class;
    }
};

// ---- the described anchor and the nearest-BEV pair IoU (what an anchor IS, given its kind row and its cell)
#define ANC_CHUNK 256
#define ANC_BOXF 6      // prepared box: x1, y1, x2, y2, area, class slot (int bits)

struct Anchor {
    float xa, ya, za, dxa, dya, dza, ra, diag;
    float x1, y1, x2, y2, area;
    int slot;
};

// the anchor of kind row `kd` at cell (x, y)
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

// ---- assignment, launch 1: boxes (rows of `row` floats, the class id last) -> aligned BEV boxes, class slots; clears the
//      per-box maxima and the positive counts
__global__ __launch_bounds__(256) void anc_prep_kernel(const float *gt, int B, int M, int row, const float *classes,
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

struct AncAssignCfg {
    int H, W, G, n_classes, M, row, code, sincos;
};

// ---- launches 2 and 3.  FINAL == false: per-box maximum.  FINAL == true: labels, targets, weights, positive counts.
template <bool FINAL, class Layout>
__global__ __launch_bounds__(256) void anc_assign_kernel(AncAssignCfg c, const float *gt, const float *pb, u32 *box_max,
                                                         const float *kinds, const float *classes, const float *shifts,
                                                         int *labels, float *reg_targets, float *reg_weights, int *gt_index,
                                                         int *num_pos) {
    __shared__ float s_kind[ANC_MAX_KINDS * Layout::KIND_F];
    __shared__ float s_box[ANC_CHUNK * ANC_BOXF];
    __shared__ int s_cnt[4];
    const int N = c.H * c.W * c.G, M = c.M;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool valid = n < N;
    stage_kinds(s_kind, kinds, c.G * Layout::KIND_F);
    const AncGeom q = Layout::geom(valid ? n : 0, c.H, c.W, c.G);
    const float *kd = s_kind + q.g * Layout::KIND_F;
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
        float t[ANC_MAX_CODE];
#pragma unroll
        for (int j = 0; j < ANC_MAX_CODE; ++j) t[j] = 0.f;
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
            if (c.sincos) {                                              // :35-38 (kind-major rows only)
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
        for (int j = 0; j < ANC_MAX_CODE; ++j)
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

// the three launches of an assignment entry (arguments checked by the caller)
template <class Layout>
void launch_assign(const AncAssignCfg &c, int batch, const float *gt, float *pb, u32 *box_max, const float *kinds,
                   const float *classes, const float *shifts, int *labels, float *reg_targets, float *reg_weights,
                   int *gt_index, int *num_pos, hipStream_t st) {
    const int prep_n = batch * c.M > batch ? batch * c.M : batch;
    anc_prep_kernel<<<pcd_div_up(prep_n, 256), 256, 0, st>>>(gt, batch, c.M, c.row, classes, c.n_classes, pb, box_max, num_pos);
    dim3 grid(pcd_div_up(c.H * c.W * c.G, 256), batch);
    anc_assign_kernel<false, Layout><<<grid, 256, 0, st>>>(c, gt, pb, box_max, kinds, classes, shifts, nullptr, nullptr, nullptr,
                                                           nullptr, nullptr);
    anc_assign_kernel<true, Layout><<<grid, 256, 0, st>>>(c, gt, pb, box_max, kinds, classes, shifts, labels, reg_targets,
                                                          reg_weights, gt_index, num_pos);
}

// ---- loss ---------------------------------------------------------------------------------------------------------------
struct AncLossCfg {
    int H, W, G, num_class, code, l1, num_bins, has_dir, sin_diff, dtype;
    float pos_w, neg_w, cls_w, loc_w, dir_w, dir_offset, two_pi, bin_period, inv_batch;
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
// heads (below) and the point heads (pointhead.hip) weight it per anchor / per point.
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

// One pass over the anchors of all heads.  GRAD == false: per-block partial sums of the three losses.  GRAD == true: the
// gradients with respect to every head's maps (every element written), scaled by the upstream gradient *grad_out.
// Anchor weights: regression and direction 1 / max(num_pos[b], 1), classification (pos_w | neg_w) / max(num_pos[b], 1)
// (anchor_head_template.py:118-120, :175-176, :211; anchor_head_multi.py:261-272; label < 0: no term at all).
// CurT == AncCurArgs (cell-major only): the positives' weights are multiplied by the (detached) curriculum weight, which
// thereby scales the focal term, the smooth-L1 weights and the direction weights (anchor_head_curriculum.py:159, :221,
// :241); CurT == AncNoCur compiles to the plain loss.
template <bool GRAD, class Layout, class CurT>
__global__ __launch_bounds__(256) void anc_loss_kernel(Layout lay, AncLossCfg c, const int *labels, const float *reg_targets,
                                                       const int *num_pos, const float *kinds, const float *code_weights,
                                                       const float *grad_out, float *partials, CurT cur) {
    __shared__ float s_kind[ANC_MAX_KINDS * Layout::KIND_F];
    __shared__ typename Layout::Shared s_lay;
    __shared__ float s_red[12];
    const int N = c.H * c.W * c.G;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    lay.stage(s_lay);
    stage_kinds(s_kind, kinds, c.G * Layout::KIND_F);
    float l_cls = 0.f, l_loc = 0.f, l_dir = 0.f;
    if (n < N) {
        const AncGeom q = Layout::geom(n, c.H, c.W, c.G);
        const AncHead &hh = lay.head(s_lay, q.g);
        const int k = q.g - hh.kind0;                                    // the anchor's kind inside its head
        const int nc = hh.num_class;
        const int label = labels[(size_t)b * N + n];
        const bool pos = label > 0;
        const float norm = fmaxf((float)num_pos[b], 1.f);
        float w = 1.f / norm;
        float wc = __fdiv_rn(pos ? c.pos_w : c.neg_w, norm);
        long long base[3];
#pragma unroll
        for (int m = 0; m < 3; ++m)
            base[m] = (long long)b * hh.strides[m][0] + (long long)q.y * hh.strides[m][2] + (long long)q.x * hh.strides[m][3];
        if constexpr (CurT::on) {
            if (pos) {
                const float x0 = load_el(hh.map[0], c.dtype, base[0] + (long long)(k * nc) * hh.strides[0][1]);
                const float cw = anc_cur_weight(cur.q, cur.saved, 1.f / (1.f + expf(-x0)), cur.groups[(size_t)b * N + n]);
                w *= cw;
                wc *= cw;
            }
        }
        float up = 0.f, upc = 0.f;
        if (GRAD) {
            up = grad_out[0] * c.inv_batch * w;
            upc = grad_out[0] * c.inv_batch * wc;
        }
        // ---- classification: sigmoid focal loss (loss_utils.py:41-74) on the head's class slice of the global one-hot
        const int tcls = pos ? (c.num_class == 1 ? 0 : label - 1) - hh.class0 : -1;   // :114-116 class agnostic
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
        // ---- regression: smooth-L1 (beta 1/9) | L1 on the codes; under sin_diff the sin-difference substitution on the
        //      heading (anchor_head_template.py:141-148, :192-193; anchor_head_multi.py:341-345)
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
            if (c.sin_diff && j == 6) {
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
        // ---- direction: cross entropy on the heading bin (:150-164, :202-216; loss_utils.py:452-469)
        if (c.has_dir) {
            const int nb = c.num_bins;
            if (!pos) {
                if (GRAD)
                    for (int j = 0; j < nb; ++j)
                        store_el(hh.grad[2], c.dtype, base[2] + (long long)(k * nb + j) * hh.strides[2][1], 0.f);
            } else {
                const float rot_gt = tg[6] + s_kind[q.g * Layout::KIND_F + K_ROT];
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

// the ordered second pass: one block, thread t sums partials t, t + 256, ... in that order (fp64), then a fixed tree
__global__ __launch_bounds__(256) void anc_loss_finish_kernel(const float *partials, int n_part, float cls_w, float loc_w,
                                                              float dir_w, float inv_batch, float *out) {
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
        const float lc = (float)(s[0][0] * inv_batch) * cls_w;
        const float ll = (float)(s[1][0] * inv_batch) * loc_w;
        const float ld = (float)(s[2][0] * inv_batch) * dir_w;
        out[0] = lc + (ll + ld);                                         // rpn_loss = cls_loss + (loc_loss + dir_loss)
        out[1] = lc;
        out[2] = ll;
        out[3] = ld;
    }
}

// forward: partials + the ordered finish (2 launches); backward: 1 launch (arguments checked by the caller)
template <class Layout, class CurT>
void launch_loss_forward(const Layout &lay, const AncLossCfg &c, dim3 grid, const int *labels, const float *reg_targets,
                         const int *num_pos, const float *kinds, const float *code_weights, float *partials, float *out,
                         const CurT &cur, hipStream_t st) {
    anc_loss_kernel<false, Layout, CurT><<<grid, 256, 0, st>>>(lay, c, labels, reg_targets, num_pos, kinds, code_weights, nullptr,
                                                               partials, cur);
    anc_loss_finish_kernel<<<1, 256, 0, st>>>(partials, (int)(grid.x * grid.y), c.cls_w, c.loc_w, c.dir_w, c.inv_batch, out);
}

// ---- decoding -----------------------------------------------------------------------------------------------------------
struct AncDecodeCfg {
    int H, W, G, n_classes, code, sincos, num_bins, has_dir, dtype;
    float dir_offset, dir_limit_offset, period;
};

// The decoded box of ONE anchor -- kind row `kd` (of the head's kind k) at cell (q.x, q.y) of frame b -- into r[0 .. code -
// sincos): box_coder_utils.py:54-77 + anchor_head_template.py:258-269.  The one copy of the decode arithmetic: the dense
// decode below and the static post-processing (anchor_postproc.hip, selected anchors only) both call it.
__device__ __forceinline__ void anc_decode_box(const AncDecodeCfg &c, const AncHead &hh, const float *kd, const float *shifts,
                                               int b, const AncGeom &q, int k, float *r /*[9]*/) {
    const Anchor a = anchor_of_kind(kd, shifts, q.x, q.y, c.W, c.H, c.n_classes);
    long long base[3];                                                   // (box and direction maps: rows 1 and 2)
#pragma unroll
    for (int m = 1; m < 3; ++m)
        base[m] = (long long)b * hh.strides[m][0] + (long long)q.y * hh.strides[m][2] + (long long)q.x * hh.strides[m][3];
    float t[ANC_MAX_CODE];
#pragma unroll
    for (int j = 0; j < ANC_MAX_CODE; ++j)
        t[j] = j < c.code ? load_el(hh.map[1], c.dtype, base[1] + (long long)(k * c.code + j) * hh.strides[1][1]) : 0.f;
    r[0] = t[0] * a.diag + a.xa;
    r[1] = t[1] * a.diag + a.ya;
    r[2] = t[2] * a.dza + a.za;
    r[3] = expf(t[3]) * a.dxa;
    r[4] = expf(t[4]) * a.dya;
    r[5] = expf(t[5]) * a.dza;
    if (c.sincos) r[6] = atan2f(t[7] + kd[K_SIN], t[6] + kd[K_COS]);     // :69-72 (kind-major rows only)
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
}

// boxes [B][N][code - sincos] and the logits as fp32 where the layout puts them
template <class Layout>
__global__ __launch_bounds__(256) void anc_decode_kernel(Layout lay, AncDecodeCfg c, const float *kinds, const float *shifts,
                                                         float *box_out) {
    __shared__ float s_kind[ANC_MAX_KINDS * Layout::KIND_F];
    __shared__ typename Layout::Shared s_lay;
    const int HW = c.H * c.W, N = HW * c.G;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    lay.stage(s_lay);
    stage_kinds(s_kind, kinds, c.G * Layout::KIND_F);
    if (n >= N) return;
    const AncGeom q = Layout::geom(n, c.H, c.W, c.G);
    const AncHead &hh = lay.head(s_lay, q.g);
    const int k = q.g - hh.kind0, nc = hh.num_class;
    const long long base0 = (long long)b * hh.strides[0][0] + (long long)q.y * hh.strides[0][2] + (long long)q.x * hh.strides[0][3];
    float *co = lay.logit_row(s_lay, hh, b, n, HW, N);
    for (int j = 0; j < nc; ++j) co[j] = load_el(hh.map[0], c.dtype, base0 + (long long)(k * nc + j) * hh.strides[0][1]);
    float r[9];
    anc_decode_box(c, hh, s_kind + q.g * Layout::KIND_F, shifts, b, q, k, r);
    const int ow = c.code - c.sincos;
    float *bo = box_out + ((size_t)b * N + n) * ow;
#pragma unroll
    for (int j = 0; j < 9; ++j)
        if (j < ow) bo[j] = r[j];
}

// ---- host-side checks and configs ---------------------------------------------------------------------------------------
bool shape_ok(int batch, int height, int width, int n_kinds, int code = 7) {
    if (batch < 1 || height < 1 || width < 1 || n_kinds < 1 || n_kinds > ANC_MAX_KINDS) return false;
    if (batch > 65535) return false;
    return (long long)batch * height * width * n_kinds * code < (1ll << 31);
}

bool bins_ok(bool has_dir, int num_dir_bins) { return !has_dir || (num_dir_bins >= 1 && num_dir_bins <= ANC_MAX_BINS); }

// One rule for "has direction maps": the config's has_dir flag; the third row of a head without them is cleared (no row of
// a descriptor is left unset).
void clear_dir_row(AncHead &h) {
    h.map[2] = nullptr;
    h.grad[2] = nullptr;
    for (int j = 0; j < 4; ++j) h.strides[2][j] = 0;
}

AncAssignCfg assign_cfg(int height, int width, int n_kinds, int n_classes, int n_boxes, int code_gt, int sincos) {
    AncAssignCfg c;
    c.H = height;
    c.W = width;
    c.G = n_kinds;
    c.n_classes = n_classes;
    c.M = n_boxes;
    c.row = code_gt + 1;
    c.code = code_gt + sincos;
    c.sincos = sincos;
    return c;
}

bool loss_cfg(AncLossCfg &c, int dtype, int batch, int height, int width, int n_kinds, int num_class, int code, int reg_l1,
              int num_dir_bins, bool has_dir, bool sin_diff, float pos_w, float neg_w, float cls_weight, float loc_weight,
              float dir_weight, float dir_offset) {
    if (dtype != PCD_F32 && dtype != PCD_BF16) return false;
    if (code < 7 || code > ANC_MAX_CODE || !shape_ok(batch, height, width, n_kinds, code)) return false;
    if (num_class < 1 || num_class > PCD_ANCHOR_MAX_CLASSES || (reg_l1 != 0 && reg_l1 != 1)) return false;
    if (!bins_ok(has_dir, num_dir_bins)) return false;
    c.H = height;
    c.W = width;
    c.G = n_kinds;
    c.num_class = num_class;
    c.code = code;
    c.l1 = reg_l1;
    c.num_bins = has_dir ? num_dir_bins : 1;
    c.has_dir = has_dir ? 1 : 0;
    c.sin_diff = sin_diff ? 1 : 0;
    c.dtype = dtype;
    c.pos_w = pos_w;
    c.neg_w = neg_w;
    c.cls_w = cls_weight;
    c.loc_w = loc_weight;
    c.dir_w = dir_weight;
    c.dir_offset = dir_offset;
    c.two_pi = (float)(2.0 * M_PI);
    c.bin_period = (float)(2.0 * M_PI / (double)c.num_bins);
    c.inv_batch = 1.0f / (float)batch;
    return true;
}

AncDecodeCfg decode_cfg(int dtype, int height, int width, int n_kinds, int n_classes, int code, int sincos, int num_dir_bins,
                        bool has_dir, float dir_offset, float dir_limit_offset) {
    AncDecodeCfg c;
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
    return c;
}

size_t assign_workspace_bytes(int batch, int n_boxes) {
    if (batch < 1 || n_boxes < 0) return 0;
    const size_t bm = (size_t)batch * (size_t)(n_boxes > 0 ? n_boxes : 1);
    return ws_piece(bm * ANC_BOXF, sizeof(float)) + ws_piece(bm, sizeof(u32));
}

size_t loss_workspace_bytes(int batch, int height, int width, int n_kinds) {
    if (!shape_ok(batch, height, width, n_kinds)) return 0;
    return ws_piece((size_t)batch * pcd_div_up(height * width * n_kinds, 256) * 3, sizeof(float));
}

// the single head's one descriptor from the three [B, H, W, C] views (strides_host: {batch, channel, y, x} x 3)
bool fill_maps(CellMajor &lay, const void *cls, const void *box, const void *dir, void *d_cls, void *d_box, void *d_dir,
               int dtype, const long long *strides_host, int n_kinds, int num_class) {
    if (!cls || !box || !strides_host || (dtype != PCD_F32 && dtype != PCD_BF16)) return false;
    AncHead &m = lay.h;
    m.map[0] = cls;
    m.map[1] = box;
    m.map[2] = dir;
    m.grad[0] = d_cls;
    m.grad[1] = d_box;
    m.grad[2] = d_dir;
    for (int q = 0; q < 3; ++q)
        for (int j = 0; j < 4; ++j) m.strides[q][j] = strides_host[q * 4 + j];
    if (!dir) clear_dir_row(m);
    m.kind0 = 0;
    m.n_kinds = n_kinds;
    m.class0 = 0;
    m.num_class = num_class;
    lay.cls_out = nullptr;
    return true;
}

// ---- the multi-head entries (anchorhead_multi.hip, anchor_multi_postproc.hip) ----------------------------------------------
bool am_code_ok(int code, int sincos) {
    const int code_gt = code - sincos;
    return (sincos == 0 || sincos == 1) && (code_gt == 7 || code_gt == 9);
}

// heads -> the kernel argument; false unless they tile the kinds [0, n_kinds) and the classes [0, num_class) in order and
// agree on the direction maps.  need_grad: the three (two) gradient pointers must be there.
bool am_fill_heads(KindMajor &hd, const PcdAnchorMultiHead *heads, int n_heads, int n_kinds, int num_class, bool need_grad,
                   bool &has_dir) {
    if (!heads || n_heads < 1 || n_heads > ANC_MAX_HEADS) return false;
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
        if (!has_dir) clear_dir_row(hd.h[h]);
        hd.cls_out[h] = nullptr;
    }
    for (int h = n_heads; h < ANC_MAX_HEADS; ++h) {
        hd.h[h] = PcdAnchorMultiHead{};
        hd.cls_out[h] = nullptr;
    }
    hd.n = n_heads;
    return kind == n_kinds && cls == num_class;
}

}  // namespace
