// AnchorHeadSingle on the device (gfx950): target assignment, fused loss, box decoding.  C ABI: include/pcd_ops.h (f3).
//
//   pcd_anchor_assign_targets   pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:36-210 for the
//                               whole batch and all anchor classes (+ pcdet/utils/box_utils.py:291-340 nearest-BEV IoU,
//                               pcdet/utils/box_coder_utils.py:13-43 ResidualCoder.encode_torch)
//   pcd_anchor_loss_forward /   pcdet/models/dense_heads/anchor_head_template.py:102-227 with pcdet/utils/loss_utils.py:
//   pcd_anchor_loss_backward    10-74 (sigmoid focal), :338-401 (weighted smooth-L1), :444-469 (weighted cross entropy)
//   pcd_anchor_decode           anchor_head_template.py:229-276 (generate_predicted_boxes) + box_coder_utils.py:45-77
//
// Anchors are never materialised: anchor n of a frame is (y, x, kind) = (n / (W * A), n / A % W, n % A), the reference's
// (y, x, class, size, rotation) order; its centre comes from the host generator's shift tables (bit-identical to the
// reference's torch.arange), its size / heading / z from the kind table.  The assignment is ANCHOR-driven: one thread per
// anchor walks the frame's boxes, staged in LDS in chunks of 256 (no cap on the number of boxes), and only divides for
// the pairs that intersect.  Three launches: box preparation, per-box maximum (integer atomic max on the bit pattern of a
// non-negative float: exact and order independent), labels + targets (the IoU recomputed with the same instructions, so
// `== maximum` means what it means in the reference).  No [N, M] matrix, no read-back.  This file is compiled with
// -ffp-contract=off (Makefile): labels depend on `==` and `>=` of fp32 values evaluated in the reference's order.
#include "anchorhead_common.h"

namespace {

// anchor n of a frame in the single head's order: (y, x, kind) = (n / (W * A), n / A % W, n % A)
__device__ __forceinline__ Anchor make_anchor(const float *s_kind, const float *shifts, int n, int A, int W, int H,
                                              int n_classes) {
    const int cell = n / A, k = n - cell * A;
    const int y = cell / W, x = cell - y * W;
    return anchor_of_kind(s_kind + k * ANC_KIND_F, shifts, x, y, W, H, n_classes);
}

// ---- launch 1: boxes -> aligned BEV boxes, class slots; clears the per-box maxima and the positive counts
__global__ __launch_bounds__(256) void anc_prep_kernel(const float *gt, int B, int M, const float *classes, int n_classes,
                                                       float *pb, u32 *box_max, int *num_pos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) num_pos[i] = 0;
    if (i >= B * M) return;
    const float *g = gt + (size_t)i * 8;
    const float pi = 3.14159265358979323846f;                          // np.pi as fp32
    const float r = g[6];
    const float ang = fabsf(r - floorf(__fdiv_rn(r, pi) + 0.5f) * pi);   // common_utils.limit_period(r, 0.5, pi).abs()
    const bool keep = ang < 0.78539816339744830962f;                   // < np.pi / 4
    const float cx = keep ? g[3] : g[4], cy = keep ? g[4] : g[3];
    const float x1 = g[0] - cx / 2.f, y1 = g[1] - cy / 2.f, x2 = g[0] + cx / 2.f, y2 = g[1] + cy / 2.f;
    const int cls = (int)g[7];
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

// ---- launches 2 and 3.  FINAL == false: per-box maximum.  FINAL == true: labels, targets, weights, positive counts.
template <bool FINAL>
__global__ __launch_bounds__(256) void anc_assign_kernel(const float *gt, const float *pb, u32 *box_max, int M, const float *kinds,
                                                         int A, const float *classes, int n_classes, const float *shifts, int W,
                                                         int H, int *labels, float *reg_targets, float *reg_weights,
                                                         int *gt_index, int *num_pos) {
    __shared__ float s_kind[ANC_MAX_KINDS * ANC_KIND_F];
    __shared__ float s_box[ANC_CHUNK * ANC_BOXF];
    __shared__ int s_cnt[4];
    const int N = H * W * A;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool valid = n < N;
    stage_kinds(s_kind, kinds, A);
    const Anchor a = make_anchor(s_kind, shifts, valid ? n : 0, A, W, H, n_classes);
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
        float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int label;
        if (forced || (arg >= 0 && best >= cl[0])) {                     // :157, :162, :188
            label = (int)cl[2];
            positive = label > 0;
        } else {
            label = best < cl[1] ? 0 : -1;                               // :164, :187
        }
        if (positive) {                                                  // box_coder_utils.py:22-43
            const float *g = gt + ((size_t)b * M + arg) * 8;
            const float dxa = fmaxf(a.dxa, 1e-5f), dya = fmaxf(a.dya, 1e-5f), dza = fmaxf(a.dza, 1e-5f);
            const float dxg = fmaxf(g[3], 1e-5f), dyg = fmaxf(g[4], 1e-5f), dzg = fmaxf(g[5], 1e-5f);
            t[0] = __fdiv_rn(g[0] - a.xa, a.diag);
            t[1] = __fdiv_rn(g[1] - a.ya, a.diag);
            t[2] = __fdiv_rn(g[2] - a.za, dza);
            t[3] = logf(__fdiv_rn(dxg, dxa));
            t[4] = logf(__fdiv_rn(dyg, dya));
            t[5] = logf(__fdiv_rn(dzg, dza));
            t[6] = g[6] - a.ra;
        }
        labels[o] = label;
#pragma unroll
        for (int j = 0; j < 7; ++j) reg_targets[o * 7 + j] = t[j];
        reg_weights[o] = positive ? 1.f : 0.f;
        if (gt_index) gt_index[o] = positive ? arg : -1;
    }
    // positives of this block -> num_pos[b] (integer atomics: order independent)
    const int wave_cnt = __popcll(__ballot(positive != 0));
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = wave_cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (c) atomicAdd(num_pos + b, c);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct AncDecodeCfg {
    int H, W, A, n_classes, num_class, num_bins;
    float dir_offset, dir_limit_offset, period;
};

__global__ __launch_bounds__(256) void anc_decode_kernel(AncMaps m, AncDecodeCfg c, const float *kinds, const float *shifts,
                                                         float *box_out, float *cls_out) {
    __shared__ float s_kind[ANC_MAX_KINDS * ANC_KIND_F];
    const int N = c.H * c.W * c.A;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    stage_kinds(s_kind, kinds, c.A);
    if (n >= N) return;
    const Anchor a = make_anchor(s_kind, shifts, n, c.A, c.W, c.H, c.n_classes);
    const int cell = n / c.A, k = n - cell * c.A;
    const int y = cell / c.W, x = cell - y * c.W;
    long long base[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) base[q] = (long long)b * m.s[q][0] + (long long)y * m.s[q][2] + (long long)x * m.s[q][3];
    const size_t o = (size_t)b * N + n;
    for (int j = 0; j < c.num_class; ++j)
        cls_out[o * c.num_class + j] = load_el(m.p[0], m.dtype, base[0] + (long long)(k * c.num_class + j) * m.s[0][1]);
    float t[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) t[j] = load_el(m.p[1], m.dtype, base[1] + (long long)(k * 7 + j) * m.s[1][1]);
    float r[7];                                                          // box_coder_utils.py:54-77
    r[0] = t[0] * a.diag + a.xa;
    r[1] = t[1] * a.diag + a.ya;
    r[2] = t[2] * a.dza + a.za;
    r[3] = expf(t[3]) * a.dxa;
    r[4] = expf(t[4]) * a.dya;
    r[5] = expf(t[5]) * a.dza;
    r[6] = t[6] + a.ra;
    if (m.p[2]) {                                                        // anchor_head_template.py:258-269
        int lab = 0;
        float mx = load_el(m.p[2], m.dtype, base[2] + (long long)(k * c.num_bins) * m.s[2][1]);
        for (int j = 1; j < c.num_bins; ++j) {
            const float v = load_el(m.p[2], m.dtype, base[2] + (long long)(k * c.num_bins + j) * m.s[2][1]);
            if (v > mx) {
                mx = v;
                lab = j;
            }
        }
        const float v = r[6] - c.dir_offset;
        const float dir_rot = v - floorf(__fdiv_rn(v, c.period) + c.dir_limit_offset) * c.period;
        r[6] = (dir_rot + c.dir_offset) + c.period * (float)lab;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) box_out[o * 7 + j] = r[j];
}


}  // namespace

extern "C" size_t pcd_anchor_assign_workspace_bytes(int batch, int n_boxes) {
    if (batch < 1 || n_boxes < 0) return 0;
    const size_t bm = (size_t)batch * (size_t)(n_boxes > 0 ? n_boxes : 1);
    return ws_piece(bm * ANC_BOXF, sizeof(float)) + ws_piece(bm, sizeof(u32));
}

extern "C" int pcd_anchor_assign_targets(const float *gt_boxes, int batch, int n_boxes, const float *kinds, int n_kinds,
                                         const float *classes, int n_classes, const float *shifts, int height, int width,
                                         int *box_cls_labels, float *box_reg_targets, float *reg_weights, int *gt_index,
                                         int *num_pos, void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    if (!kinds || !classes || !shifts || !box_cls_labels || !box_reg_targets || !reg_weights || !num_pos || n_boxes < 0 ||
        (n_boxes > 0 && !gt_boxes))
        return PCD_ERR_INVALID_ARG;
    if (!shape_ok(batch, height, width, n_kinds) || n_classes < 1 || n_classes > ANC_MAX_CLASSES ||
        (long long)batch * n_boxes >= (1ll << 27))
        return PCD_ERR_UNSUPPORTED;
    WsCarver ws(workspace, workspace_bytes);
    const size_t bm = (size_t)batch * (size_t)(n_boxes > 0 ? n_boxes : 1);
    float *pb = ws.take<float>(bm * ANC_BOXF);
    u32 *box_max = ws.take<u32>(bm);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int N = height * width * n_kinds;
    const int prep_n = batch * n_boxes > batch ? batch * n_boxes : batch;
    anc_prep_kernel<<<pcd_div_up(prep_n, 256), 256, 0, st>>>(gt_boxes, batch, n_boxes, classes, n_classes, pb, box_max, num_pos);
    dim3 grid(pcd_div_up(N, 256), batch);
    anc_assign_kernel<false><<<grid, 256, 0, st>>>(gt_boxes, pb, box_max, n_boxes, kinds, n_kinds, classes, n_classes, shifts,
                                                   width, height, nullptr, nullptr, nullptr, nullptr, nullptr);
    anc_assign_kernel<true><<<grid, 256, 0, st>>>(gt_boxes, pb, box_max, n_boxes, kinds, n_kinds, classes, n_classes, shifts,
                                                  width, height, box_cls_labels, box_reg_targets, reg_weights, gt_index, num_pos);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" size_t pcd_anchor_loss_workspace_bytes(int batch, int height, int width, int n_kinds) {
    if (!shape_ok(batch, height, width, n_kinds)) return 0;
    return ws_piece((size_t)batch * pcd_div_up(height * width * n_kinds, 256) * 3, sizeof(float));
}

extern "C" int pcd_anchor_loss_forward(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                                       const long long *strides_host, const int *box_cls_labels, const float *box_reg_targets,
                                       const int *num_pos, int batch, int height, int width, int n_kinds, int num_class,
                                       int num_dir_bins, const float *kinds, const float *code_weights, float cls_weight,
                                       float loc_weight, float dir_weight, float dir_offset, float *out, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    AncMaps m;
    AncLossCfg c;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, nullptr, nullptr, nullptr, dtype, strides_host) || !box_cls_labels ||
        !box_reg_targets || !num_pos || !kinds || !code_weights || !out)
        return PCD_ERR_INVALID_ARG;
    if (!loss_cfg(c, batch, height, width, n_kinds, num_class, num_dir_bins, dir_preds != nullptr, cls_weight, loc_weight,
                  dir_weight, dir_offset))
        return PCD_ERR_UNSUPPORTED;
    WsCarver ws(workspace, workspace_bytes);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    float *partials = ws.take<float>((size_t)grid.x * grid.y * 3);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    anc_loss_kernel<false, AncNoCur><<<grid, 256, 0, st>>>(m, c, box_cls_labels, box_reg_targets, num_pos, kinds, code_weights, nullptr,
                                                           partials, AncNoCur());
    anc_loss_finish_kernel<<<1, 256, 0, st>>>(partials, (int)(grid.x * grid.y), c, out);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_loss_backward(const void *cls_preds, const void *box_preds, const void *dir_preds, void *d_cls,
                                        void *d_box, void *d_dir, int dtype, const long long *strides_host,
                                        const int *box_cls_labels, const float *box_reg_targets, const int *num_pos, int batch,
                                        int height, int width, int n_kinds, int num_class, int num_dir_bins, const float *kinds,
                                        const float *code_weights, float cls_weight, float loc_weight, float dir_weight,
                                        float dir_offset, const float *grad_out, void *stream) {
    PCD_ENTER();
    AncMaps m;
    AncLossCfg c;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, d_cls, d_box, d_dir, dtype, strides_host) || !d_cls || !d_box ||
        (dir_preds && !d_dir) || !box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights || !grad_out)
        return PCD_ERR_INVALID_ARG;
    if (!loss_cfg(c, batch, height, width, n_kinds, num_class, num_dir_bins, dir_preds != nullptr, cls_weight, loc_weight,
                  dir_weight, dir_offset))
        return PCD_ERR_UNSUPPORTED;
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    anc_loss_kernel<true, AncNoCur><<<grid, 256, 0, (hipStream_t)stream>>>(m, c, box_cls_labels, box_reg_targets, num_pos, kinds,
                                                                 code_weights, grad_out, nullptr, AncNoCur());
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_decode(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                                 const long long *strides_host, int batch, int height, int width, int n_kinds, int n_classes,
                                 int num_class, int num_dir_bins, const float *kinds, const float *shifts, float dir_offset,
                                 float dir_limit_offset, float *batch_box_preds, float *batch_cls_preds, void *stream) {
    PCD_ENTER();
    AncMaps m;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, nullptr, nullptr, nullptr, dtype, strides_host) || !kinds || !shifts ||
        !batch_box_preds || !batch_cls_preds)
        return PCD_ERR_INVALID_ARG;
    if (!shape_ok(batch, height, width, n_kinds) || n_classes < 1 || n_classes > ANC_MAX_CLASSES || num_class < 1 ||
        num_class > PCD_ANCHOR_MAX_CLASSES || (dir_preds && (num_dir_bins < 1 || num_dir_bins > ANC_MAX_BINS)) ||
        (long long)batch * height * width * n_kinds * num_class >= (1ll << 31))
        return PCD_ERR_UNSUPPORTED;
    AncDecodeCfg c;
    c.H = height;
    c.W = width;
    c.A = n_kinds;
    c.n_classes = n_classes;
    c.num_class = num_class;
    c.num_bins = dir_preds ? num_dir_bins : 1;
    c.dir_offset = dir_offset;
    c.dir_limit_offset = dir_limit_offset;
    c.period = (float)(2.0 * M_PI / (double)c.num_bins);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    anc_decode_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(m, c, kinds, shifts, batch_box_preds, batch_cls_preds);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
