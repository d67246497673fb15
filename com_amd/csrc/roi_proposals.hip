// The two static halves of a two-stage detector's eval forward for gfx950, both on the shared selection core
// (postproc_common.h) exactly as anchor_postproc.hip is: an argument struct with a key producer, the core's fill ... gather
// launches, a finish kernel of its own, the core's NMS mask / reduce, and one output kernel (the core's pads labels with 0 and
// knows no cls / iou score columns).  Fixed launches, no host read-back, grids from the shapes alone.  C ABI:
// include/pcd_ops.h (f4c, f4d).
//
// pcd_anchor_proposals (f4c) replaces RoIHeadTemplate.proposal_layer (roi_head_template.py:45-102) over
// AnchorHeadTemplate.generate_predicted_boxes (anchor_head_template.py:229-276) WITHOUT its output: no [B, N, 7] and no
// [B, N, num_class] tensor; only the <= NMS_PRE_MAXSIZE selected anchors of a frame are decoded.  One problem per frame,
// element i = anchor n = (y * W + x) * A + kind:
//   score   the raw logit (bf16 widened first): the maximum of the anchor's num_class logits, label = the lowest class index
//           that attains it, + 1.  No sigmoid: roi_scores are logits (cls_preds_normalized is False)
//   pass    every anchor; a NaN maximum never takes part
//   order   score descending, then n ascending
//   11 launches: fill, keys, find 1, hist 2, find 2, ties, gather | finish (sort, label, decode) | nms mask, nms reduce | output
//
// pcd_roi_postproc (f4d) replaces the class-agnostic branch of Detector3DTemplate.post_processing
// (detector3d_template.py:178-290) and SECONDNetIoU.post_processing (second_net_iou.py:75-177) over class_agnostic_nms
// (model_nms_utils.py:6-25).  One problem per frame over ALL its R RoI rows:
//   score   one block per frame writes score / cls / iou [B][R] into the workspace first (score_by_class needs the number of
//           distinct labels of the frame), so the key producer is one load
//   pass    score >= SCORE_THRESH, inclusive; every row without one; a NaN never
//   order   score descending, then row ascending
//   12 launches: scores | the 7 of the core | finish (sort, gather rows) | nms mask, nms reduce | output
//
// The key of both: logits are negative as a rule and composed scores can be, so the bits(score) + 1 of anchor_postproc.hip
// does not order them.  ordered_key() is the usual order-preserving map of the f32 bits (sign bit set for positives, all bits
// flipped for negatives) after -0.0 -> +0.0; its smallest value, for -inf, is 0x007fffff, so 0 is free for "NaN: never".
// score >= t is then key >= ordered_key(t), i.e. (long long)key > ordered_key(t) - 1: the `key > thr` rule of the core.
// No float atomics; workgroups never hand data to each other inside a launch.
#include "anchorhead_common.h"
#include "postproc_common.h"

namespace {

__host__ __device__ __forceinline__ u32 ordered_bits(u32 b) {
    if (b == 0x80000000u) b = 0u;                        // -0.0 == +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u32 ordered_key(float s) { return s != s ? 0u : ordered_bits(__float_as_uint(s)); }

// nms mask + nms reduce of the core (pp_launch_nms_output without its output kernel)
void rp_launch_nms(int K, int pre, int cbk, float nms_thresh, unsigned P, bool normal, const PpBuffers &w, hipStream_t st) {
    const dim3 tiles((unsigned)cbk, (unsigned)cbk, P);
    if (cbk > 0) {
        if (normal) pp_nms_mask_kernel<true><<<tiles, 64, 0, st>>>(K, 7, pre, cbk, nms_thresh, w.sbox, w.scount, w.mask);
        else pp_nms_mask_kernel<false><<<tiles, 64, 0, st>>>(K, 7, pre, cbk, nms_thresh, w.sbox, w.scount, w.mask);
    }
    pp_nms_reduce_kernel<<<P, 64, 0, st>>>(K, pre, cbk, w.mask, w.scount, w.keep, w.nkeep);
}

// per frame: the first `post` kept rows in keep order; behind them boxes 0, scores 0, labels `pad_label`.  xa / xb: two more
// sorted score columns [P][K] -> oa / ob [P][post] (NULL: none).
__global__ __launch_bounds__(PP_THREADS) void rp_output_kernel(int K, int post, long long pad_label, const float *__restrict__ sbox,
                                                               const float *__restrict__ sscore, const int *__restrict__ scls,
                                                               const float *__restrict__ xa, const float *__restrict__ xb,
                                                               const int *__restrict__ keep, const int *__restrict__ nkeep,
                                                               float *__restrict__ boxes, float *__restrict__ scores,
                                                               long long *__restrict__ labels, int32_t *__restrict__ count,
                                                               float *__restrict__ oa, float *__restrict__ ob) {
    const int p = blockIdx.x;
    const int k = min(nkeep[p], post);
    const int *kp = keep + (size_t)p * K;
    const size_t o0 = (size_t)p * post;
    for (int j = threadIdx.x; j < post; j += PP_THREADS) {
        const bool live = j < k;
        const size_t q = (size_t)p * K + (live ? kp[j] : 0);
        for (int d = 0; d < 7; ++d) boxes[(o0 + j) * 7 + d] = live ? sbox[q * 7 + d] : 0.f;
        scores[o0 + j] = live ? sscore[q] : 0.f;
        labels[o0 + j] = live ? (long long)scls[q] : pad_label;
        if (oa) oa[o0 + j] = live ? xa[q] : 0.f;
        if (ob) ob[o0 + j] = live ? xb[q] : 0.f;
    }
    if (threadIdx.x == 0) count[p] = k;
}

// ---- f4c: the proposal layer -------------------------------------------------------------------------------------------------
struct PrArgs {
    AncHead h;                                 // the three maps and their element strides {batch, channel, y, x}
    AncDecodeCfg dc;
    const float *kinds, *shifts;
    int B, H, W, G, nc, K, KP2, pre, post, chw_max, nchunks, cbk;
    long long thr;
    float nms_thresh;

    // maximum logit and its 0-based label of anchor n of frame b
    __device__ __forceinline__ float score(int b, int n, int &label) const {
        const AncGeom q = CellMajor::geom(n, H, W, G);
        const long long off = (long long)b * h.strides[0][0] + (long long)q.y * h.strides[0][2] +
                              (long long)q.x * h.strides[0][3] + (long long)(q.g * nc) * h.strides[0][1];
        float best = 0.f;
        int lab = 0;
        for (int j = 0; j < nc; ++j) {         // (j ascending: `>` keeps the lowest index of a tie; a NaN stays)
            const float s = load_el(h.map[0], dc.dtype, off + (long long)j * h.strides[0][1]);
            if (j == 0 || s > best || (s != s && best == best)) {
                best = s;
                lab = j;
            }
        }
        label = lab;
        return best;
    }
    __device__ __forceinline__ int count(int) const { return chw_max; }
    __device__ __forceinline__ u32 key(int p, int i) const {
        int label;
        return ordered_key(score(p, i, label));
    }
};

// sort (score desc, n asc), label, decode: sbox [B][K][7], sscore (the logit itself), scls (1-based label), scount
__global__ __launch_bounds__(PP_THREADS) void pr_finish_kernel(PrArgs a, const u64 *__restrict__ cand, const u32 *__restrict__ cand_n,
                                                               float *__restrict__ sbox, float *__restrict__ sscore,
                                                               int *__restrict__ scls, int *__restrict__ scount) {
    extern __shared__ u64 srt[];                         // [KP2]
    __shared__ float s_kind[ANC_MAX_KINDS * CellMajor::KIND_F];
    const int p = blockIdx.x;
    stage_kinds(s_kind, a.kinds, a.G * CellMajor::KIND_F);
    const int n = sel_load_sort(cand, cand_n, p, a.K, a.KP2, srt);
    float *bp = sbox + (size_t)p * a.K * 7;
    float *sp = sscore + (size_t)p * a.K;
    int *cl = scls + (size_t)p * a.K;
    for (int j = threadIdx.x; j < n; j += PP_THREADS) {
        const int i = (int)(0xffffffffu - (u32)srt[j]);
        // (read again, at most K anchors per frame: the key folds -0.0 into +0.0, the output keeps the logit's own bits)
        int label;
        const float s = a.score(p, i, label);
        const AncGeom q = CellMajor::geom(i, a.H, a.W, a.G);
        float r[9];
        anc_decode_box(a.dc, a.h, s_kind + q.g * CellMajor::KIND_F, a.shifts, p, q, q.g, r);
#pragma unroll
        for (int d = 0; d < 7; ++d) bp[(size_t)j * 7 + d] = r[d];
        sp[j] = s;
        cl[j] = label + 1;
    }
    if (threadIdx.x == 0) scount[p] = n;
}

int pr_setup(const PcdAnchorProposalsConfig *cfg, PrArgs &a) {
    if (!cfg) return PCD_ERR_INVALID_ARG;
    const PcdAnchorProposalsConfig &c = *cfg;
    if (c.nms_normal != 0 && c.nms_normal != 1) return PCD_ERR_INVALID_ARG;
    if (c.batch < 1 || c.height < 1 || c.width < 1 || c.nms_pre < 1 || c.nms_post < 1 || c.batch > 65535) return PCD_ERR_UNSUPPORTED;
    if (c.n_kinds < 1 || c.n_kinds > ANC_MAX_KINDS || c.n_classes < 1 || c.n_classes > ANC_MAX_CLASSES || c.num_class < 1 ||
        c.num_class > PCD_ANCHOR_MAX_CLASSES || c.nms_pre > PCD_POSTPROC_MAX_K)
        return PCD_ERR_UNSUPPORTED;
    const long long N = (long long)c.height * c.width * c.n_kinds;
    if (N >= 0x7fffffffLL - PP_CHUNK) return PCD_ERR_UNSUPPORTED;           // flat index must fit int32
    a = PrArgs{};
    a.B = c.batch;
    a.H = c.height;
    a.W = c.width;
    a.G = c.n_kinds;
    a.nc = c.num_class;
    a.K = (int)(N < c.nms_pre ? N : c.nms_pre);
    a.KP2 = 1;
    while (a.KP2 < a.K) a.KP2 <<= 1;
    a.pre = a.K;
    a.post = c.nms_post;
    a.chw_max = (int)N;
    a.nchunks = pcd_div_up(a.chw_max, PP_CHUNK);
    a.cbk = pcd_div_up(a.K, 64);
    a.thr = 0;                                                              // every anchor whose score is not NaN
    a.nms_thresh = c.nms_thresh;
    return PCD_OK;
}

// ---- f4d: the post-processing of a RoI head ------------------------------------------------------------------------------------
struct RpArgs {
    const float *wscore;                       // [B][R]: the NMS scores of rp_scores_kernel
    int R, K, KP2, pre, post, chw_max, nchunks, cbk;
    long long thr;
    float nms_thresh;
    __device__ __forceinline__ int count(int) const { return R; }
    __device__ __forceinline__ u32 key(int p, int i) const { return ordered_key(wscore[(size_t)p * R + i]); }
};

// one block per frame: wscore / wcls / wiou [B][R]
__global__ __launch_bounds__(PP_THREADS) void rp_scores_kernel(PcdRoiPostprocConfig c, const float *__restrict__ iou_in,
                                                               const float *__restrict__ cls_in, const long long *__restrict__ roi_labels,
                                                               const int32_t *__restrict__ point_counts, float *__restrict__ wscore,
                                                               float *__restrict__ wcls, float *__restrict__ wiou) {
    __shared__ int present[PCD_POSTPROC_MAX_CLASSES + 1];
    __shared__ int s_distinct;
    const int b = blockIdx.x, R = c.rois;
    const size_t r0 = (size_t)b * R;
    const bool labelled = c.has_class_labels && roi_labels;
    int distinct = 0;
    if (c.score_type == PCD_ROIPP_SCORE_BY_CLASS) {        // the reference's len(label_preds.unique()) over the clamped labels
        if (threadIdx.x <= PCD_POSTPROC_MAX_CLASSES) present[threadIdx.x] = 0;
        __syncthreads();
        for (int r = threadIdx.x; r < R; r += PP_THREADS) {
            const long long l = labelled ? roi_labels[r0 + r] : 1;
            present[(int)(l < 0 ? 0 : (l > c.num_class ? c.num_class : l))] = 1;       // (every writer stores the same 1)
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int d = 0;
            for (int j = 0; j <= c.num_class; ++j) d += present[j];
            s_distinct = d;
        }
        __syncthreads();
        distinct = s_distinct;
    }
    for (int r = threadIdx.x; r < R; r += PP_THREADS) {
        const float x = iou_in[r0 + r];
        const float iou = c.normalized ? x : sigmoid_f32(x);
        float cls = 0.f;
        if (c.score_type != PCD_ROIPP_SCORE_RCNN) {
            const float y = cls_in[r0 + r];
            cls = c.normalized ? y : sigmoid_f32(y);
        }
        float s;
        switch (c.score_type) {
        case PCD_ROIPP_SCORE_CLS: s = cls; break;
        case PCD_ROIPP_SCORE_WEIGHTED: {
            const float u = c.weight_iou * iou, v = c.weight_cls * cls;
            s = u + v;
            break;
        }
        case PCD_ROIPP_SCORE_BY_CLASS: {
            const long long l0 = labelled ? roi_labels[r0 + r] : 1;
            const int l = (int)(l0 < 0 ? 0 : (l0 > c.num_class ? c.num_class : l0));
            s = (l >= 1 && l <= distinct) ? (c.by_class_iou[l - 1] ? iou : cls) : 0.f;
            break;
        }
        case PCD_ROIPP_SCORE_NUM_PTS: {
            const float n = (float)point_counts[r0 + r];
            const float inv = 1.0f / c.pts_span;         // (a tensor over a host scalar: torch multiplies by the reciprocal)
            const float ramp = (n - 10.f) * inv;
            const float alpha = n >= c.pts_iou_thresh ? 1.f : (n > c.pts_cls_thresh ? ramp : 0.f);
            const float u = (1.f - alpha) * cls, v = alpha * iou;
            s = u + v;
            break;
        }
        default: s = iou; break;                         // PCD_ROIPP_SCORE_RCNN, PCD_ROIPP_SCORE_IOU
        }
        wscore[r0 + r] = s;
        wcls[r0 + r] = cls;
        wiou[r0 + r] = iou;
    }
}

// sort (score desc, row asc), gather the rows: sbox, sscore, scls (output label), xcls / xiou, scount
__global__ __launch_bounds__(PP_THREADS) void rp_finish_kernel(RpArgs a, int labelled, const u64 *__restrict__ cand,
                                                               const u32 *__restrict__ cand_n, const float *__restrict__ box_in,
                                                               const long long *__restrict__ roi_labels, const float *__restrict__ wcls,
                                                               const float *__restrict__ wiou, float *__restrict__ sbox,
                                                               float *__restrict__ sscore, int *__restrict__ scls,
                                                               float *__restrict__ xcls, float *__restrict__ xiou,
                                                               int *__restrict__ scount) {
    extern __shared__ u64 srt[];                         // [KP2]
    const int p = blockIdx.x;
    const int n = sel_load_sort(cand, cand_n, p, a.K, a.KP2, srt);
    const size_t r0 = (size_t)p * a.R, k0 = (size_t)p * a.K;
    for (int j = threadIdx.x; j < n; j += PP_THREADS) {
        const int i = (int)(0xffffffffu - (u32)srt[j]);
#pragma unroll
        for (int d = 0; d < 7; ++d) sbox[(k0 + j) * 7 + d] = box_in[(r0 + i) * 7 + d];
        sscore[k0 + j] = a.wscore[r0 + i];
        scls[k0 + j] = labelled ? (int)roi_labels[r0 + i] : 1;
        xcls[k0 + j] = wcls[r0 + i];
        xiou[k0 + j] = wiou[r0 + i];
    }
    if (threadIdx.x == 0) scount[p] = n;
}

struct RpLayout {
    PpLayout core;
    size_t o_wscore, o_wcls, o_wiou, o_xcls, o_xiou, total;
};

int rp_setup(const PcdRoiPostprocConfig *cfg, RpArgs &a, RpLayout &l) {
    if (!cfg) return PCD_ERR_INVALID_ARG;
    const PcdRoiPostprocConfig &c = *cfg;
    if (c.nms_normal != 0 && c.nms_normal != 1) return PCD_ERR_INVALID_ARG;
    if (c.batch < 1 || c.batch > 65535 || c.rois < 1 || c.rois > PCD_POSTPROC_MAX_K || c.nms_pre < 1 || c.nms_post < 1)
        return PCD_ERR_UNSUPPORTED;
    if (c.score_type < PCD_ROIPP_SCORE_RCNN || c.score_type > PCD_ROIPP_SCORE_NUM_PTS) return PCD_ERR_UNSUPPORTED;
    if (c.score_type == PCD_ROIPP_SCORE_BY_CLASS && (c.num_class < 1 || c.num_class > PCD_POSTPROC_MAX_CLASSES))
        return PCD_ERR_UNSUPPORTED;
    if (c.score_type == PCD_ROIPP_SCORE_NUM_PTS && !(c.pts_iou_thresh >= c.pts_cls_thresh)) return PCD_ERR_UNSUPPORTED;
    a = RpArgs{};
    a.R = c.rois;
    a.K = c.rois < c.nms_pre ? c.rois : c.nms_pre;
    a.KP2 = 1;
    while (a.KP2 < a.K) a.KP2 <<= 1;
    a.pre = a.K;
    a.post = c.nms_post;
    a.chw_max = c.rois;
    a.nchunks = pcd_div_up(a.chw_max, PP_CHUNK);
    a.cbk = pcd_div_up(a.K, 64);
    const float t = c.score_thresh;
    if (!c.use_score_thresh) a.thr = 0;                                     // every row whose score is not NaN
    else if (t != t) a.thr = 0xffffffffLL;                                  // score >= NaN: nothing
    else a.thr = (long long)ordered_bits(__builtin_bit_cast(u32, t)) - 1;
    a.nms_thresh = c.nms_thresh;
    const size_t P = (size_t)c.batch;
    l.core = pp_layout(P, a.K, 7, a.chw_max, a.nchunks, a.cbk);
    size_t off = l.core.total;
    auto take = [&](size_t bytes) { const size_t o = off; off += pcd_align_up(bytes, 256); return o; };
    l.o_wscore = take(P * a.R * 4);
    l.o_wcls = take(P * a.R * 4);
    l.o_wiou = take(P * a.R * 4);
    l.o_xcls = take(P * a.K * 4);
    l.o_xiou = take(P * a.K * 4);
    l.total = off;
    return PCD_OK;
}

}  // namespace

extern "C" size_t pcd_anchor_proposals_workspace_bytes(const PcdAnchorProposalsConfig *cfg) {
    PrArgs a;
    if (pr_setup(cfg, a) != PCD_OK) return 0;
    return pp_layout((size_t)a.B, a.K, 7, a.chw_max, a.nchunks, a.cbk).total;
}

extern "C" int pcd_anchor_proposals(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                                    const long long *strides_host, const float *kinds, const float *shifts,
                                    const PcdAnchorProposalsConfig *cfg, float *rois, float *roi_scores, long long *roi_labels,
                                    int32_t *count, void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    PrArgs a;
    const int rc = pr_setup(cfg, a);
    if (rc != PCD_OK) return rc;
    CellMajor m;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, nullptr, nullptr, nullptr, dtype, strides_host, cfg->n_kinds,
                   cfg->num_class) ||
        !kinds || !shifts || !rois || !roi_scores || !roi_labels || !count)
        return PCD_ERR_INVALID_ARG;
    for (int q = 0; q < 3; ++q)
        for (int j = 0; j < 4; ++j)
            if (m.h.strides[q][j] < 0) return PCD_ERR_INVALID_ARG;
    if (!bins_ok(dir_preds != nullptr, cfg->num_dir_bins)) return PCD_ERR_UNSUPPORTED;
    a.h = m.h;
    a.dc = decode_cfg(dtype, a.H, a.W, a.G, cfg->n_classes, 7, 0, cfg->num_dir_bins, dir_preds != nullptr, cfg->dir_offset,
                      cfg->dir_limit_offset);
    a.kinds = kinds;
    a.shifts = shifts;
    const unsigned P = (unsigned)a.B;
    const PpLayout l = pp_layout(P, a.K, 7, a.chw_max, a.nchunks, a.cbk);
    if (!workspace || workspace_bytes < l.total || ((uintptr_t)workspace & 255)) return PCD_ERR_WORKSPACE;
    const PpBuffers w = pp_buffers(workspace, l);
    hipStream_t st = (hipStream_t)stream;
    pp_launch_select(a, P, workspace, l, w, st);
    pr_finish_kernel<<<P, PP_THREADS, (size_t)a.KP2 * sizeof(u64), st>>>(a, w.cand, w.cand_n, w.sbox, w.sscore, w.scls, w.scount);
    rp_launch_nms(a.K, a.pre, a.cbk, a.nms_thresh, P, cfg->nms_normal != 0, w, st);
    rp_output_kernel<<<P, PP_THREADS, 0, st>>>(a.K, a.post, 1, w.sbox, w.sscore, w.scls, nullptr, nullptr, w.keep, w.nkeep, rois,
                                               roi_scores, roi_labels, count, nullptr, nullptr);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" size_t pcd_roi_postproc_workspace_bytes(const PcdRoiPostprocConfig *cfg) {
    RpArgs a;
    RpLayout l;
    if (rp_setup(cfg, a, l) != PCD_OK) return 0;
    return l.total;
}

extern "C" int pcd_roi_postproc(const float *batch_box_preds, const float *batch_cls_preds, const float *roi_scores,
                                const long long *roi_labels, const int32_t *point_counts, const PcdRoiPostprocConfig *cfg,
                                float *boxes, float *scores, long long *labels, int32_t *count, float *cls_scores,
                                float *iou_scores, void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    RpArgs a;
    RpLayout l;
    const int rc = rp_setup(cfg, a, l);
    if (rc != PCD_OK) return rc;
    const bool rcnn = cfg->score_type == PCD_ROIPP_SCORE_RCNN;
    if (!batch_box_preds || !batch_cls_preds || !boxes || !scores || !labels || !count) return PCD_ERR_INVALID_ARG;
    if ((!rcnn && !roi_scores) || (cfg->has_class_labels && !roi_labels)) return PCD_ERR_INVALID_ARG;
    if (rcnn ? (cls_scores || iou_scores) : (!cls_scores || !iou_scores)) return PCD_ERR_INVALID_ARG;
    if (cfg->score_type == PCD_ROIPP_SCORE_NUM_PTS && !point_counts) return PCD_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < l.total || ((uintptr_t)workspace & 255)) return PCD_ERR_WORKSPACE;
    const unsigned P = (unsigned)cfg->batch;
    const PpBuffers w = pp_buffers(workspace, l.core);
    char *ws = (char *)workspace;
    float *wscore = (float *)(ws + l.o_wscore), *wcls = (float *)(ws + l.o_wcls), *wiou = (float *)(ws + l.o_wiou);
    float *xcls = (float *)(ws + l.o_xcls), *xiou = (float *)(ws + l.o_xiou);
    a.wscore = wscore;
    hipStream_t st = (hipStream_t)stream;
    rp_scores_kernel<<<P, PP_THREADS, 0, st>>>(*cfg, batch_cls_preds, roi_scores, roi_labels, point_counts, wscore, wcls, wiou);
    pp_launch_select(a, P, workspace, l.core, w, st);
    rp_finish_kernel<<<P, PP_THREADS, (size_t)a.KP2 * sizeof(u64), st>>>(a, cfg->has_class_labels != 0, w.cand, w.cand_n,
                                                                         batch_box_preds, roi_labels, wcls, wiou, w.sbox, w.sscore,
                                                                         w.scls, xcls, xiou, w.scount);
    rp_launch_nms(a.K, a.pre, a.cbk, a.nms_thresh, P, cfg->nms_normal != 0, w, st);
    rp_output_kernel<<<P, PP_THREADS, 0, st>>>(a.K, a.post, 0, w.sbox, w.sscore, w.scls, rcnn ? nullptr : xcls,
                                               rcnn ? nullptr : xiou, w.keep, w.nkeep, boxes, scores, labels, count, cls_scores,
                                               iou_scores);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
