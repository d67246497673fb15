// Static post-processing of CenterPoint-style heads for gfx950: top-K selection, box decoding, masking, class-agnostic NMS
// and the per-frame gather of every (frame, head) "problem" of a batch in a fixed number of launches, with no host read-back
// and grids that depend on the shapes only -- so the whole chain sits inside a captured inference graph.
// Replaces CenterHead.generate_predicted_boxes (center_head.py:266-317) -> centernet_utils.decode_bbox_from_heatmap
// (centernet_utils.py:199-257) -> model_nms_utils.class_agnostic_nms (model_nms_utils.py:15-27) -> nms_gpu /
// nms_normal_gpu (iou3d_nms_utils.py:85-116).
//
// Order of the selection (total, documented in include/pcd_ops.h): score = fp32 sigmoid of the map value, descending; equal
// scores by flat index c*H*W + y*W + x ascending.  A score is a non-negative float, so its bit pattern orders like the score
// and (bits << 32) | (0xffffffff - index) is one unique 64-bit key per pixel; the selection finds the K-th largest key.
//
// Launches (P = frames x heads problems, grids from the shapes alone):
//   fill      zero the histograms and candidate counters
//   keys      chunks x P blocks: score bits of every pixel -> keys[], histogram of the high 16 bits of the passing ones
//   find 1    P blocks: the bin of the K-th largest key (or "all pass" when fewer than K pass SCORE_THRESH)
//   hist 2    chunks x P: histogram of the low 16 bits inside that bin
//   find 2    P blocks: the exact score bits T of the K-th key, how many ties at T are still taken (r)
//   ties      chunks x P: the number of pixels with bits == T per chunk (chunks are index ranges)
//   gather    chunks x P: every key > T and the first r ties by index (chunk prefix + ordered block scan) -> candidates
//   finish    P blocks: sort the <= K candidates in LDS, decode, limit-range mask, ballot compaction in score order
//   nms mask  tiles x tiles x P waves: suppression bits over the first min(count, NMS_PRE_MAXSIZE) boxes (blocks beyond exit)
//   nms red.  P waves: the greedy keep list
//   output    B blocks: heads concatenated in head order, NMS_POST_MAXSIZE per head, zeros behind count
// Workgroups never hand data to each other inside a launch: every hand-over is a launch boundary.  The only atomics are
// integer adds (histograms, candidate slots); the candidates are sorted by their unique keys, so slot order never shows.
// Every launch but `finish` is the shared core of postproc_common.h (also under anchor_postproc.hip); this file holds the
// centre heads' key producer (PpArgs::key), their finish kernel and the entry points.
#include "postproc_common.h"

namespace {

constexpr int PP_MAPS = 6;                     // hm, center, center_z, dim, rot, vel

struct PpMap {
    const void *p;
    int s[4];                                  // element strides (B, C, H, W)
    int bf16;
};
struct PpHead {
    PpMap m[PP_MAPS];
    int C;
    int label[PCD_POSTPROC_MAX_CLASSES];
};
struct PpArgs {
    PpHead h[PCD_POSTPROC_MAX_HEADS];
    int B, NH, H, W, K, KP2, pre, post, D, chw_max, nchunks, cbk;
    long long thr;                             // a pixel passes SCORE_THRESH iff (long long)bits > thr (-1: every pixel)
    float limit[6];
    float fstride, vx, vy, px, py, nms_thresh;
    // the key producer of the shared core (postproc_common.h): problem p = (frame, head), element i = c*H*W + y*W + x,
    // key = bits of sigmoid(hm) (a non-negative float: its bit pattern orders like the score)
    __device__ __forceinline__ int count(int p) const { return h[p % NH].C * H * W; }
    __device__ __forceinline__ u32 key(int p, int i) const;
    __device__ __forceinline__ int out_label(int hd, int c) const { return h[hd].label[c]; }
};
__device__ __forceinline__ float ld_map(const PpMap &m, int b, int c, int y, int x) {
    const long long off = (long long)b * m.s[0] + (long long)c * m.s[1] + (long long)y * m.s[2] + (long long)x * m.s[3];
    return load_el(m.p, m.bf16 ? PCD_BF16 : PCD_F32, off);
}
__device__ __forceinline__ u32 PpArgs::key(int p, int i) const {
    const int hw = H * W, c = i / hw, rem = i - c * hw, y = rem / W, x = rem - y * W;
    return __float_as_uint(sigmoid_f32(ld_map(h[p % NH].m[0], p / NH, c, y, x)));
}

// sort (score desc, index asc), decode (centernet_utils.py:217-257), POST_CENTER_LIMIT_RANGE, compaction in score order
__global__ __launch_bounds__(PP_THREADS) void pp_finish_kernel(PpArgs a, const u64 *__restrict__ cand, const u32 *__restrict__ cand_n,
                                                               float *__restrict__ sbox, float *__restrict__ sscore,
                                                               int *__restrict__ scls, int *__restrict__ scount) {
    extern __shared__ u64 srt[];                         // [KP2]
    __shared__ int lds[4];
    const int p = blockIdx.x;
    const int n = sel_load_sort(cand, cand_n, p, a.K, a.KP2, srt);
    const PpHead &hd = a.h[p % a.NH];
    const int b = p / a.NH, hw = a.H * a.W, D = a.D;
    float *bp = sbox + (size_t)p * a.K * D;
    float *sp = sscore + (size_t)p * a.K;
    int *cl = scls + (size_t)p * a.K;
    int base = 0;
    for (int j0 = 0; j0 < n; j0 += PP_THREADS) {
        const int j = j0 + threadIdx.x;
        float box[9] = {};
        float score = 0.f;
        int c = 0;
        bool valid = false;
        if (j < n) {
            const u64 k64 = srt[j];
            const int i = (int)(0xffffffffu - (u32)k64);
            score = __uint_as_float((u32)(k64 >> 32));
            c = i / hw;
            const int rem = i - c * hw, y = rem / a.W, x = rem - y * a.W;
            const float xs = (float)x + ld_map(hd.m[1], b, 0, y, x);
            const float ys = (float)y + ld_map(hd.m[1], b, 1, y, x);
            box[0] = xs * a.fstride * a.vx + a.px;
            box[1] = ys * a.fstride * a.vy + a.py;
            box[2] = ld_map(hd.m[2], b, 0, y, x);
            box[3] = expf(ld_map(hd.m[3], b, 0, y, x));
            box[4] = expf(ld_map(hd.m[3], b, 1, y, x));
            box[5] = expf(ld_map(hd.m[3], b, 2, y, x));
            box[6] = atan2f(ld_map(hd.m[4], b, 1, y, x), ld_map(hd.m[4], b, 0, y, x));
            if (D == 9) {
                box[7] = ld_map(hd.m[5], b, 0, y, x);
                box[8] = ld_map(hd.m[5], b, 1, y, x);
            }
            valid = box[0] >= a.limit[0] && box[1] >= a.limit[1] && box[2] >= a.limit[2] &&
                    box[0] <= a.limit[3] && box[1] <= a.limit[4] && box[2] <= a.limit[5];
        }
        int total;
        const int pos = base + block_exclusive_scan(valid ? 1 : 0, lds, total);
        if (valid) {
#pragma unroll
            for (int d = 0; d < 9; ++d)
                if (d < D) bp[(size_t)pos * D + d] = box[d];
            sp[pos] = score;
            cl[pos] = c;
        }
        base += total;
    }
    if (threadIdx.x == 0) scount[p] = base;
}

// validation + kernel arguments; 0 when the configuration is refused
int pp_setup(const PcdPostprocHead *heads, const PcdPostprocConfig *cfg, PpArgs &a) {
    if (!heads || !cfg) return PCD_ERR_INVALID_ARG;
    const PcdPostprocConfig &c = *cfg;
    if (c.batch <= 0 || c.num_heads <= 0 || c.height <= 0 || c.width <= 0 || c.max_obj <= 0 || c.nms_pre <= 0 ||
        c.nms_post <= 0 || (c.nms_normal != 0 && c.nms_normal != 1))
        return PCD_ERR_INVALID_ARG;
    if (c.num_heads > PCD_POSTPROC_MAX_HEADS || c.max_obj > PCD_POSTPROC_MAX_K || c.nms_pre > PCD_POSTPROC_MAX_K)
        return PCD_ERR_UNSUPPORTED;
    if ((long long)c.batch * c.num_heads > 65535) return PCD_ERR_UNSUPPORTED;
    a = PpArgs{};
    a.B = c.batch;
    a.NH = c.num_heads;
    a.H = c.height;
    a.W = c.width;
    a.K = c.max_obj;
    a.KP2 = 1;
    while (a.KP2 < a.K) a.KP2 <<= 1;
    a.pre = c.nms_pre < a.K ? c.nms_pre : a.K;
    a.post = c.nms_post;
    a.cbk = pcd_div_up(a.K, 64);
    const bool vel = heads[0].map[5] != nullptr;
    a.D = vel ? 9 : 7;
    long long chw_max = 0;
    const int chans[PP_MAPS] = {0, 2, 1, 3, 2, 2};
    for (int h = 0; h < a.NH; ++h) {
        const PcdPostprocHead &s = heads[h];
        if (s.num_class <= 0 || s.num_class > PCD_POSTPROC_MAX_CLASSES) return PCD_ERR_UNSUPPORTED;
        if ((s.map[5] != nullptr) != vel) return PCD_ERR_INVALID_ARG;
        const long long chw = (long long)s.num_class * a.H * a.W;
        if (chw >= 0x7fffffffLL - PP_CHUNK) return PCD_ERR_UNSUPPORTED;     // flat index must fit int32
        chw_max = chw > chw_max ? chw : chw_max;
        a.h[h].C = s.num_class;
        for (int k = 0; k < PCD_POSTPROC_MAX_CLASSES; ++k) a.h[h].label[k] = s.label[k];
        for (int m = 0; m < PP_MAPS; ++m) {
            if (m == 5 && !vel) continue;
            if (!s.map[m] || (s.dtype[m] != PCD_F32 && s.dtype[m] != PCD_BF16)) return PCD_ERR_INVALID_ARG;
            const int extent[4] = {a.B, m == 0 ? s.num_class : chans[m], a.H, a.W};
            long long last = 0;
            for (int d = 0; d < 4; ++d) {
                if (s.strides[m][d] < 0) return PCD_ERR_INVALID_ARG;
                last += s.strides[m][d] * (extent[d] - 1);
            }
            if (last >= 0x7fffffffLL) return PCD_ERR_UNSUPPORTED;          // strides kept as int32 on the device
            a.h[h].m[m].p = s.map[m];
            for (int d = 0; d < 4; ++d) a.h[h].m[m].s[d] = (int)s.strides[m][d];
            a.h[h].m[m].bf16 = s.dtype[m] == PCD_BF16;
        }
    }
    a.chw_max = (int)chw_max;
    a.nchunks = pcd_div_up(a.chw_max, PP_CHUNK);
    a.thr = c.use_score_thresh && c.score_thresh >= 0.f ? (long long)__builtin_bit_cast(u32, c.score_thresh) : -1;
    for (int k = 0; k < 6; ++k) a.limit[k] = c.limit[k];
    a.fstride = c.feature_map_stride;
    a.vx = c.voxel_x;
    a.vy = c.voxel_y;
    a.px = c.pc_x;
    a.py = c.pc_y;
    a.nms_thresh = c.nms_thresh;
    return PCD_OK;
}

}  // namespace

extern "C" size_t pcd_centerhead_postproc_workspace_bytes(const PcdPostprocHead *heads, const PcdPostprocConfig *cfg) {
    PpArgs a;
    if (pp_setup(heads, cfg, a) != PCD_OK) return 0;
    return pp_layout((size_t)a.B * a.NH, a.K, a.D, a.chw_max, a.nchunks, a.cbk).total;
}

extern "C" int pcd_centerhead_postproc(const PcdPostprocHead *heads, const PcdPostprocConfig *cfg, float *boxes, float *scores,
                                       long long *labels, int32_t *count, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    PCD_ENTER();
    PpArgs a;
    const int rc = pp_setup(heads, cfg, a);
    if (rc != PCD_OK) return rc;
    if (!boxes || !scores || !labels || !count) return PCD_ERR_INVALID_ARG;
    const unsigned P = (unsigned)(a.B * a.NH);
    const PpLayout l = pp_layout(P, a.K, a.D, a.chw_max, a.nchunks, a.cbk);
    if (!workspace || workspace_bytes < l.total || ((uintptr_t)workspace & 255)) return PCD_ERR_WORKSPACE;
    const PpBuffers w = pp_buffers(workspace, l);
    hipStream_t st = (hipStream_t)stream;
    pp_launch_select(a, P, workspace, l, w, st);
    pp_finish_kernel<<<P, PP_THREADS, (size_t)a.KP2 * sizeof(u64), st>>>(a, w.cand, w.cand_n, w.sbox, w.sscore, w.scls, w.scount);
    pp_launch_nms_output(a, P, (unsigned)a.B, cfg->nms_normal != 0, w, boxes, scores, labels, count, st);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
