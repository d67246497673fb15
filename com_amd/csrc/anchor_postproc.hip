// Static post-processing of AnchorHeadSingle for gfx950: score + label, top-K selection, box decoding of the selected anchors
// and class-agnostic NMS for every frame of a batch in a fixed number of launches, with no host read-back and grids that
// depend on the shapes only -- so the chain sits inside a captured inference graph.  C ABI: include/pcd_ops.h (f4a).
// Replaces Detector3DTemplate.post_processing (detector3d_template.py:178-290, the single-head class-agnostic branch) ->
// model_nms_utils.class_agnostic_nms (model_nms_utils.py:6-25) over the output of AnchorHeadTemplate.
// generate_predicted_boxes (anchor_head_template.py:229-276), WITHOUT that output: no [B, N, 7] and no [B, N, num_class]
// tensor is written; only the <= NMS_PRE_MAXSIZE selected anchors of a frame are decoded.
//
// One selection problem per frame (the NMS is class-agnostic), element i = anchor n = (y * W + x) * A + kind.
//   score   score_c = fp32 sigmoid of the class logit (bf16 widened first), the anchor's score = the maximum over its
//           num_class scores, its label = the lowest class index that attains it, + 1
//   pass    score >= SCORE_THRESH (inclusive, model_nms_utils.py:9); every anchor without a threshold; a NaN score never
//   order   score descending, then n ascending (total; torch.topk leaves ties unordered)
// A score is a float in [0, 1], so bits(score) + 1 orders like the score, is never 0 and leaves 0 for "NaN: never passes";
// score >= t is then key > bits(t) for t > 0 and key > 0 for t <= 0 or no threshold -- the `(long long)key > thr` rule of the
// shared selection core (postproc_common.h), whose launches, sort, NMS and output kernels this file uses as they are:
//   fill, keys, find 1, hist 2, find 2, ties, gather    (postproc_common.h; the key producer is ApArgs::key below)
//   finish    B blocks: sort the <= K candidates in LDS, label + decode (anc_decode_box of anchorhead_common.h: the device
//             function pcd_anchor_decode's kernel calls, hence its bits)
//   nms mask, nms reduce, output                        (postproc_common.h)
// 11 launches.  No float atomics; workgroups never hand data to each other inside a launch.
#include "anchorhead_common.h"
#include "postproc_common.h"

namespace {

struct ApArgs {
    AncHead h;                                 // the three maps and their element strides {batch, channel, y, x}
    AncDecodeCfg dc;
    const float *kinds, *shifts;
    int B, NH, H, W, G, nc, K, KP2, pre, post, D, chw_max, nchunks, cbk;
    int cls_pairs;                             // bf16 logits with channel stride 1: an anchor's classes are adjacent elements
    long long thr;                             // an anchor passes iff (long long)key > thr
    float nms_thresh;

    // score and 0-based label of anchor n of frame b
    __device__ __forceinline__ float score(int b, int n, int &label) const {
        const AncGeom q = CellMajor::geom(n, H, W, G);
        const long long off = (long long)b * h.strides[0][0] + (long long)q.y * h.strides[0][2] +
                              (long long)q.x * h.strides[0][3] + (long long)(q.g * nc) * h.strides[0][1];
        float best = 0.f;
        int lab = 0;
        auto feed = [&](int j, float logit) {  // (j ascending: `>` keeps the lowest index of a tie; a NaN stays)
            const float s = sigmoid_f32(logit);
            if (j == 0 || s > best || (s != s && best == best)) {
                best = s;
                lab = j;
            }
        };
        if (cls_pairs) {                       // aligned pairs as one 32-bit load, a single element at an odd end
            const unsigned short *e = (const unsigned short *)h.map[0] + off;
            int j = 0;
            if ((uintptr_t)e & 2) {
                feed(0, bf16_bits_to_f32(e[0]));
                j = 1;
            }
            for (; j + 1 < nc; j += 2) {
                const u32 w = *(const u32 *)(e + j);
                feed(j, __uint_as_float(w << 16));
                feed(j + 1, __uint_as_float(w & 0xffff0000u));
            }
            if (j < nc) feed(j, bf16_bits_to_f32(e[j]));
        } else {
            for (int j = 0; j < nc; ++j) feed(j, load_el(h.map[0], dc.dtype, off + (long long)j * h.strides[0][1]));
        }
        label = lab;
        return best;
    }
    // the key producer of the shared core
    __device__ __forceinline__ int count(int) const { return chw_max; }
    __device__ __forceinline__ u32 key(int p, int i) const {
        int label;
        const float s = score(p, i, label);
        return s != s ? 0u : __float_as_uint(s) + 1u;
    }
    __device__ __forceinline__ int out_label(int, int c) const { return c; }
};

// sort (score desc, n asc), label, decode: sbox [B][K][7], sscore, scls (1-based label), scount
__global__ __launch_bounds__(PP_THREADS) void ap_finish_kernel(ApArgs a, const u64 *__restrict__ cand, const u32 *__restrict__ cand_n,
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
        const u64 k64 = srt[j];
        const int i = (int)(0xffffffffu - (u32)k64);
        // The label is recomputed through the SIGMOIDS, deliberately: it is the lowest class at the maximum SCORE, and two
        // different logits can share a score (both saturate to 1.0), so an argmax over the logits would name another class.
        // At most K anchors per frame pay this second read.
        int label;
        a.score(p, i, label);
        const AncGeom q = CellMajor::geom(i, a.H, a.W, a.G);
        float r[9];
        anc_decode_box(a.dc, a.h, s_kind + q.g * CellMajor::KIND_F, a.shifts, p, q, q.g, r);
#pragma unroll
        for (int d = 0; d < 7; ++d) bp[(size_t)j * 7 + d] = r[d];
        sp[j] = __uint_as_float((u32)(k64 >> 32) - 1u);
        cl[j] = label + 1;
    }
    if (threadIdx.x == 0) scount[p] = n;
}

// validation + kernel arguments (maps left unset)
int ap_setup(const PcdAnchorPostprocConfig *cfg, ApArgs &a) {
    if (!cfg) return PCD_ERR_INVALID_ARG;
    const PcdAnchorPostprocConfig &c = *cfg;
    if (c.nms_normal != 0 && c.nms_normal != 1) return PCD_ERR_INVALID_ARG;
    if (c.batch < 1 || c.height < 1 || c.width < 1 || c.nms_pre < 1 || c.nms_post < 1 || c.batch > 65535) return PCD_ERR_UNSUPPORTED;
    if (c.n_kinds < 1 || c.n_kinds > ANC_MAX_KINDS || c.n_classes < 1 || c.n_classes > ANC_MAX_CLASSES || c.num_class < 1 ||
        c.num_class > PCD_ANCHOR_MAX_CLASSES || c.nms_pre > PCD_POSTPROC_MAX_K)
        return PCD_ERR_UNSUPPORTED;
    const long long N = (long long)c.height * c.width * c.n_kinds;
    if (N >= 0x7fffffffLL - PP_CHUNK) return PCD_ERR_UNSUPPORTED;           // flat index must fit int32
    a = ApArgs{};
    a.B = c.batch;
    a.NH = 1;
    a.H = c.height;
    a.W = c.width;
    a.G = c.n_kinds;
    a.nc = c.num_class;
    a.K = c.nms_pre;
    a.KP2 = 1;
    while (a.KP2 < a.K) a.KP2 <<= 1;
    a.pre = a.K;
    a.post = c.nms_post;
    a.D = 7;
    a.chw_max = (int)N;
    a.nchunks = pcd_div_up(a.chw_max, PP_CHUNK);
    a.cbk = pcd_div_up(a.K, 64);
    const float t = c.score_thresh;
    if (!c.use_score_thresh || t <= 0.f) a.thr = 0;                         // every anchor whose score is not NaN
    else if (t != t) a.thr = 0xffffffffLL;                                  // score >= NaN: nothing
    else a.thr = (long long)__builtin_bit_cast(u32, t);
    a.nms_thresh = c.nms_thresh;
    return PCD_OK;
}

}  // namespace

extern "C" size_t pcd_anchor_postproc_workspace_bytes(const PcdAnchorPostprocConfig *cfg) {
    ApArgs a;
    if (ap_setup(cfg, a) != PCD_OK) return 0;
    return pp_layout((size_t)a.B, a.K, a.D, a.chw_max, a.nchunks, a.cbk).total;
}

extern "C" int pcd_anchor_postproc(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                                   const long long *strides_host, const float *kinds, const float *shifts,
                                   const PcdAnchorPostprocConfig *cfg, float *boxes, float *scores, long long *labels,
                                   int32_t *count, void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    ApArgs a;
    const int rc = ap_setup(cfg, a);
    if (rc != PCD_OK) return rc;
    CellMajor m;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, nullptr, nullptr, nullptr, dtype, strides_host, cfg->n_kinds,
                   cfg->num_class) ||
        !kinds || !shifts || !boxes || !scores || !labels || !count)
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
    a.cls_pairs = dtype == PCD_BF16 && m.h.strides[0][1] == 1 && ((uintptr_t)cls_preds & 1) == 0;
    const unsigned P = (unsigned)a.B;
    const PpLayout l = pp_layout(P, a.K, a.D, a.chw_max, a.nchunks, a.cbk);
    if (!workspace || workspace_bytes < l.total || ((uintptr_t)workspace & 255)) return PCD_ERR_WORKSPACE;
    const PpBuffers w = pp_buffers(workspace, l);
    hipStream_t st = (hipStream_t)stream;
    pp_launch_select(a, P, workspace, l, w, st);
    ap_finish_kernel<<<P, PP_THREADS, (size_t)a.KP2 * sizeof(u64), st>>>(a, w.cand, w.cand_n, w.sbox, w.sscore, w.scls, w.scount);
    pp_launch_nms_output(a, P, P, cfg->nms_normal != 0, w, boxes, scores, labels, count, st);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
