// Static post-processing of AnchorHeadMulti for gfx950: per-class score, top-K selection, box decoding of the selected anchors
// and per-class NMS for every frame of a batch in a fixed number of launches, with no host read-back and grids that depend on
// the shapes only -- so the chain sits inside a captured inference graph.  C ABI: include/pcd_ops.h (f4b).
// Replaces the MULTI_CLASSES_NMS branch of Detector3DTemplate.post_processing (detector3d_template.py:224-249) ->
// model_nms_utils.multi_classes_nms (model_nms_utils.py:28-66) over the output of AnchorHeadTemplate.generate_predicted_boxes
// with use_multihead (anchor_head_template.py:229-276), WITHOUT that output: no [B, N, D] and no [B, N_h, C_h] tensor is
// written; only the <= NMS_PRE_MAXSIZE selected anchors of a (frame, class) pair are decoded.
//
// One selection problem per (frame, class): p = b * num_class + c, c the GLOBAL class index; head h owns the classes
// [class0_h, class0_h + num_class_h), k = c - class0_h.  The elements of p are the local anchors i in [0, N_h) of that head,
// N_h = n_kinds_h * H * W, i = (a * H + y) * W + x with a the head-local kind -- the row order of batch_cls_preds[h]; the
// global anchor is n = kind0_h * H * W + i.  count(p) = N_h, chw_max = the largest N_h.
//   score   fp32 sigmoid of the logit at channel a * num_class_h + k of head h's cls map, cell (y, x) (bf16 widened first)
//   pass    score >= SCORE_THRESH (inclusive, model_nms_utils.py:42); every non-NaN score without a threshold; a NaN never
//   order   score descending, then i ascending (total; torch.topk leaves ties unordered)
//   select  the first min(NMS_PRE_MAXSIZE, passing) elements
//   decode  only the selected anchors, anc_decode_box under the KindMajor geometry of n (anchorhead_common.h: the device
//           function pcd_anchor_multi_decode's kernel calls, hence its bits), D = code - sincos columns; an anchor selected
//           under two classes of one head is decoded twice and appears twice, as in the reference
//   nms     nms_gpu / nms_normal_gpu on columns 0:7 in that order, the first NMS_POST_MAXSIZE survivors
//   output  per frame the problems' survivors in global class order = head order, then class order inside the head
//           (detector3d_template.py:233-249); label = the per-class table (multihead_label_mapping[h][k]); zeros behind count
// The key encoding is anchor_postproc.hip's: bits(score) + 1, 0 for NaN; score >= t is `(long long)key > thr`, the rule of the
// shared selection core (postproc_common.h), whose launches, sort, NMS and output kernels this file uses as they are:
//   fill, keys, find 1, hist 2, find 2, ties, gather    (postproc_common.h; the key producer is AmpArgs::key below)
//   finish    P blocks: sort the <= K candidates in LDS, decode, label
//   nms mask, nms reduce, output                        (postproc_common.h; NH = num_class problems per frame)
// 11 launches.  No float atomics; workgroups never hand data to each other inside a launch.
// Kernel arguments: AmpArgs carries the 8 head descriptors by value (8 x 160 B) + tables: about 1.5 KB, under the 4 KB limit.
// LDS of the finish kernel: 8 B x next power of two of K for the sort (32 KB at K = 4096) + the kind rows (1.5 KB) + the
// problem's head descriptor: within 64 KB.
#include "anchorhead_common.h"
#include "postproc_common.h"

namespace {

struct AmpArgs {
    AncHead h[ANC_MAX_HEADS];                  // the three maps of every head and their element strides {batch, channel, y, x}
    AncDecodeCfg dc;
    const float *kinds, *shifts;
    int B, NH, H, W, HW, K, KP2, pre, post, D, chw_max, nchunks, cbk;      // NH = num_class: the problems of a frame
    long long thr;                             // an element passes iff (long long)key > thr
    float nms_thresh;
    int label[ANC_MAX_CLASSES];                // output label of global class c
    unsigned char head_of_class[ANC_MAX_CLASSES];

    // the key producer of the shared core (p is uniform over a block: the head is read through scalar loads)
    __device__ __forceinline__ int count(int p) const {
        const int c = p % NH;
        return h[head_of_class[c]].n_kinds * HW;
    }
    __device__ __forceinline__ u32 key(int p, int i) const {
        const int b = p / NH, c = p - b * NH;
        const AncHead &hh = h[head_of_class[c]];
        const int a = i / HW, cell = i - a * HW;
        const int y = cell / W, x = cell - y * W;
        const long long off = (long long)b * hh.strides[0][0] + (long long)y * hh.strides[0][2] + (long long)x * hh.strides[0][3] +
                              (long long)(a * hh.num_class + (c - hh.class0)) * hh.strides[0][1];
        const float s = sigmoid_f32(load_el(hh.map[0], dc.dtype, off));
        return s != s ? 0u : __float_as_uint(s) + 1u;
    }
    __device__ __forceinline__ int out_label(int, int c) const { return c; }   // (the finish kernel stored the label itself)
};

// sort (score desc, i asc), decode, label: sbox [P][K][D], sscore, scls (the output label), scount
__global__ __launch_bounds__(PP_THREADS) void amp_finish_kernel(AmpArgs a, const u64 *__restrict__ cand, const u32 *__restrict__ cand_n,
                                                                float *__restrict__ sbox, float *__restrict__ sscore,
                                                                int *__restrict__ scls, int *__restrict__ scount) {
    extern __shared__ u64 srt[];                         // [KP2]
    __shared__ float s_kind[ANC_MAX_KINDS * KindMajor::KIND_F];
    __shared__ AncHead s_head;                           // the head of this problem's class
    const int p = blockIdx.x;
    const int b = p / a.NH, c = p - b * a.NH;
    if (threadIdx.x == 0) s_head = a.h[a.head_of_class[c]];
    stage_kinds(s_kind, a.kinds, a.dc.G * KindMajor::KIND_F);
    const int n = sel_load_sort(cand, cand_n, p, a.K, a.KP2, srt);
    const AncHead &hh = s_head;
    const int D = a.D, label = a.label[c];
    float *bp = sbox + (size_t)p * a.K * D;
    float *sp = sscore + (size_t)p * a.K;
    int *cl = scls + (size_t)p * a.K;
    for (int j = threadIdx.x; j < n; j += PP_THREADS) {
        const u64 k64 = srt[j];
        const int i = (int)(0xffffffffu - (u32)k64);
        const int k = i / a.HW, cell = i - k * a.HW;     // the anchor's kind inside its head
        AncGeom q;
        q.g = hh.kind0 + k;
        q.y = cell / a.W;
        q.x = cell - q.y * a.W;
        float r[9];
        anc_decode_box(a.dc, hh, s_kind + q.g * KindMajor::KIND_F, a.shifts, b, q, k, r);
#pragma unroll
        for (int d = 0; d < 9; ++d)
            if (d < D) bp[(size_t)j * D + d] = r[d];
        sp[j] = __uint_as_float((u32)(k64 >> 32) - 1u);
        cl[j] = label;
    }
    if (threadIdx.x == 0) scount[p] = n;
}

// validation + kernel arguments
int amp_setup(const PcdAnchorMultiHead *heads, int n_heads, const PcdAnchorMultiPostprocConfig *cfg, AmpArgs &a) {
    if (!cfg || !heads) return PCD_ERR_INVALID_ARG;
    const PcdAnchorMultiPostprocConfig &c = *cfg;
    if (c.nms_normal != 0 && c.nms_normal != 1) return PCD_ERR_INVALID_ARG;
    if (c.nms_pre < 1 || c.nms_post < 1 || c.nms_pre > PCD_POSTPROC_MAX_K) return PCD_ERR_UNSUPPORTED;
    if (c.batch < 1 || c.height < 1 || c.width < 1 || c.n_kinds < 1 || c.n_kinds > ANC_MAX_KINDS || !am_code_ok(c.code, c.sincos) ||
        c.n_classes < 1 || c.n_classes > ANC_MAX_CLASSES || c.num_class < 1 || c.num_class > PCD_ANCHOR_MAX_CLASSES)
        return PCD_ERR_UNSUPPORTED;
    if ((long long)c.height * c.width * c.n_kinds >= 0x7fffffffLL - PP_CHUNK) return PCD_ERR_UNSUPPORTED;   // flat index: int32
    if ((long long)c.batch * c.num_class > 65535) return PCD_ERR_UNSUPPORTED;          // P: a grid's y / z extent
    KindMajor hd;
    bool has_dir = false;
    if (!am_fill_heads(hd, heads, n_heads, c.n_kinds, c.num_class, false, has_dir)) return PCD_ERR_INVALID_ARG;
    if (!bins_ok(has_dir, c.num_dir_bins)) return PCD_ERR_UNSUPPORTED;
    a = AmpArgs{};
    int kinds_max = 0;
    for (int h = 0; h < n_heads; ++h) {
        a.h[h] = hd.h[h];
        for (int q = 0; q < 3; ++q)
            for (int j = 0; j < 4; ++j)
                if (a.h[h].strides[q][j] < 0) return PCD_ERR_INVALID_ARG;
        for (int k = 0; k < a.h[h].num_class; ++k) a.head_of_class[a.h[h].class0 + k] = (unsigned char)h;
        kinds_max = a.h[h].n_kinds > kinds_max ? a.h[h].n_kinds : kinds_max;
    }
    for (int k = 0; k < c.num_class; ++k) a.label[k] = c.label[k];
    a.B = c.batch;
    a.NH = c.num_class;
    a.H = c.height;
    a.W = c.width;
    a.HW = c.height * c.width;
    a.K = c.nms_pre;
    a.KP2 = 1;
    while (a.KP2 < a.K) a.KP2 <<= 1;
    a.pre = a.K;
    a.post = c.nms_post;
    a.D = c.code - c.sincos;
    a.chw_max = a.HW * kinds_max;
    a.nchunks = pcd_div_up(a.chw_max, PP_CHUNK);
    a.cbk = pcd_div_up(a.K, 64);
    const float t = c.score_thresh;
    if (!c.use_score_thresh || t <= 0.f) a.thr = 0;                         // every element whose score is not NaN
    else if (t != t) a.thr = 0xffffffffLL;                                  // score >= NaN: nothing
    else a.thr = (long long)__builtin_bit_cast(u32, t);
    a.nms_thresh = c.nms_thresh;
    a.dc = decode_cfg(PCD_F32, a.H, a.W, c.n_kinds, c.n_classes, c.code, c.sincos, c.num_dir_bins, has_dir, c.dir_offset,
                      c.dir_limit_offset);
    return PCD_OK;
}

}  // namespace

extern "C" size_t pcd_anchor_multi_postproc_workspace_bytes(const PcdAnchorMultiHead *heads, int n_heads,
                                                            const PcdAnchorMultiPostprocConfig *cfg) {
    AmpArgs a;
    if (amp_setup(heads, n_heads, cfg, a) != PCD_OK) return 0;
    return pp_layout((size_t)a.B * a.NH, a.K, a.D, a.chw_max, a.nchunks, a.cbk).total;
}

extern "C" int pcd_anchor_multi_postproc(const PcdAnchorMultiHead *heads, int n_heads, int dtype, const float *kinds,
                                         const float *shifts, const PcdAnchorMultiPostprocConfig *cfg, float *boxes,
                                         float *scores, long long *labels, int32_t *count, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    AmpArgs a;
    const int rc = amp_setup(heads, n_heads, cfg, a);
    if (rc != PCD_OK) return rc;
    if ((dtype != PCD_F32 && dtype != PCD_BF16) || !kinds || !shifts || !boxes || !scores || !labels || !count)
        return PCD_ERR_INVALID_ARG;
    a.dc.dtype = dtype;
    a.kinds = kinds;
    a.shifts = shifts;
    const unsigned P = (unsigned)(a.B * a.NH);
    const PpLayout l = pp_layout(P, a.K, a.D, a.chw_max, a.nchunks, a.cbk);
    if (!workspace || workspace_bytes < l.total || ((uintptr_t)workspace & 255)) return PCD_ERR_WORKSPACE;
    const PpBuffers w = pp_buffers(workspace, l);
    hipStream_t st = (hipStream_t)stream;
    pp_launch_select(a, P, workspace, l, w, st);
    amp_finish_kernel<<<P, PP_THREADS, (size_t)a.KP2 * sizeof(u64), st>>>(a, w.cand, w.cand_n, w.sbox, w.sscore, w.scls, w.scount);
    pp_launch_nms_output(a, P, (unsigned)a.B, cfg->nms_normal != 0, w, boxes, scores, labels, count, st);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
