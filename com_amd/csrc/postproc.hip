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
#include "common.h"
#include "iou3d_geom.h"

namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_CHUNK = 2048;                 // pixels per block of the streaming launches (8 per thread)
constexpr int PP_BINS = 65536;                 // 16-bit digits
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
};
// per-problem selection state (find launches -> later launches)
struct PpSel {
    int all;                                   // fewer than K pass: take every passing pixel
    int b1;                                    // high digit of the cut
    int above;                                 // keys above the cut's bin (pass 1), above T (pass 2)
    int r;                                     // ties at T still taken
    long long T;                               // take key > T (+ the first r with key == T)
    long long pad;
};

__device__ __forceinline__ float ld_map(const PpMap &m, int b, int c, int y, int x) {
    const long long off = (long long)b * m.s[0] + (long long)c * m.s[1] + (long long)y * m.s[2] + (long long)x * m.s[3];
    return load_el(m.p, m.bf16 ? PCD_BF16 : PCD_F32, off);
}

// one atomic per distinct bin of the wave (all-equal scores -- fresh weights -- would otherwise serialise on one address)
__device__ __forceinline__ void wave_hist_add(u32 *hist, bool active, u32 bin) {
    u64 todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const u32 lb = (u32)__shfl((int)bin, leader, 64);
        const u64 same = __ballot(active && bin == lb) & todo;
        if (lane_id() == leader) atomicAdd(hist + lb, (u32)__popcll(same));
        todo &= ~same;
    }
}

__device__ __forceinline__ int problem_chw(const PpArgs &a, int p) { return a.h[p % a.NH].C * a.H * a.W; }

// keys[p][i] = bits of sigmoid(hm); hist1[p][bits >> 16] counts the pixels that pass SCORE_THRESH
__global__ __launch_bounds__(PP_THREADS) void pp_keys_kernel(PpArgs a, u32 *__restrict__ keys, u32 *__restrict__ hist1) {
    const int p = blockIdx.y, chw = problem_chw(a, p);
    const int i0 = blockIdx.x * PP_CHUNK;
    if (i0 >= chw) return;
    const PpMap &hm = a.h[p % a.NH].m[0];
    const int b = p / a.NH, hw = a.H * a.W;
    u32 *kp = keys + (size_t)p * a.chw_max;
    u32 *hp = hist1 + (size_t)p * PP_BINS;
    for (int e = 0; e < PP_CHUNK; e += PP_THREADS) {
        const int i = i0 + e + threadIdx.x;
        const bool in = i < chw;
        u32 key = 0;
        if (in) {
            const int c = i / hw, rem = i - c * hw, y = rem / a.W, x = rem - y * a.W;
            key = __float_as_uint(sigmoid_f32(ld_map(hm, b, c, y, x)));
            kp[i] = key;
        }
        wave_hist_add(hp, in && (long long)key > a.thr, key >> 16);
    }
}

// The bin holding the `need`-th largest counted key: thread t owns bins of group 255 - t (thread 0 the highest), an exclusive
// scan over the threads gives the count above each group, the one thread whose group crosses `need` walks its bins.
__device__ void find_cut(const u32 *__restrict__ hist, int need, int *lds, int &bin_out, int &above_out) {
    const int g = PP_THREADS - 1 - (int)threadIdx.x, per = PP_BINS / PP_THREADS;
    const u32 *hg = hist + (size_t)g * per;
    int sum = 0;
    for (int j = 0; j < per; ++j) sum += (int)hg[j];
    int total;
    const int above = block_exclusive_scan(sum, lds, total);
    if (above < need && above + sum >= need) {
        int acc = above;
        for (int j = per - 1; j >= 0; --j) {
            const int c = (int)hg[j];
            if (acc + c >= need) {
                lds[4] = g * per + j;
                lds[5] = acc;
                break;
            }
            acc += c;
        }
    }
    __syncthreads();
    bin_out = lds[4];
    above_out = lds[5];
}

__global__ __launch_bounds__(PP_THREADS) void pp_find1_kernel(PpArgs a, const u32 *__restrict__ hist1, PpSel *__restrict__ sel) {
    __shared__ int lds[8];
    const int p = blockIdx.x;
    const u32 *hp = hist1 + (size_t)p * PP_BINS;
    int sum = 0;
    for (int j = threadIdx.x; j < PP_BINS; j += PP_THREADS) sum += (int)hp[j];
    int total;
    block_exclusive_scan(sum, lds, total);
    if (total <= a.K) {                                  // every passing pixel is selected
        if (threadIdx.x == 0) {
            PpSel s = {};
            s.all = 1;
            s.T = a.thr;
            s.above = total;
            sel[p] = s;
        }
        return;
    }
    int bin, above;
    find_cut(hp, a.K, lds, bin, above);
    if (threadIdx.x == 0) {
        PpSel s = {};
        s.all = 0;
        s.b1 = bin;
        s.above = above;
        sel[p] = s;
    }
}

// low 16 bits of the passing keys inside the cut's bin
__global__ __launch_bounds__(PP_THREADS) void pp_hist2_kernel(PpArgs a, const u32 *__restrict__ keys, const PpSel *__restrict__ sel,
                                                              u32 *__restrict__ hist2) {
    const int p = blockIdx.y, chw = problem_chw(a, p);
    const int i0 = blockIdx.x * PP_CHUNK;
    const PpSel s = sel[p];
    if (i0 >= chw || s.all) return;
    const u32 *kp = keys + (size_t)p * a.chw_max;
    u32 *hp = hist2 + (size_t)p * PP_BINS;
    for (int e = 0; e < PP_CHUNK; e += PP_THREADS) {
        const int i = i0 + e + threadIdx.x;
        const u32 key = i < chw ? kp[i] : 0u;
        wave_hist_add(hp, i < chw && (long long)key > a.thr && (int)(key >> 16) == s.b1, key & 0xffffu);
    }
}

__global__ __launch_bounds__(PP_THREADS) void pp_find2_kernel(PpArgs a, const u32 *__restrict__ hist2, PpSel *__restrict__ sel) {
    __shared__ int lds[8];
    const int p = blockIdx.x;
    const PpSel s = sel[p];
    if (s.all) return;
    int bin, above;
    find_cut(hist2 + (size_t)p * PP_BINS, a.K - s.above, lds, bin, above);
    if (threadIdx.x == 0) {
        PpSel o = s;
        o.T = ((long long)s.b1 << 16) | bin;
        o.above = s.above + above;                       // keys > T
        o.r = a.K - o.above;                             // >= 1 ties at T taken
        sel[p] = o;
    }
}

// pixels with key == T per chunk
__global__ __launch_bounds__(PP_THREADS) void pp_ties_kernel(PpArgs a, const u32 *__restrict__ keys, const PpSel *__restrict__ sel,
                                                             int *__restrict__ ties) {
    __shared__ int lds[4];
    const int p = blockIdx.y, chw = problem_chw(a, p);
    const int i0 = blockIdx.x * PP_CHUNK;
    const PpSel s = sel[p];
    if (i0 >= chw || s.all) return;
    const u32 *kp = keys + (size_t)p * a.chw_max;
    int n = 0;
    for (int e = 0; e < PP_CHUNK; e += PP_THREADS) {
        const int i = i0 + e + threadIdx.x;
        n += (i < chw && (long long)kp[i] == s.T) ? 1 : 0;
    }
    int total;
    block_exclusive_scan(n, lds, total);
    if (threadIdx.x == 0) ties[(size_t)p * a.nchunks + blockIdx.x] = total;
}

// candidates: keys > T, and the ties at T whose rank in index order is below r
__global__ __launch_bounds__(PP_THREADS) void pp_gather_kernel(PpArgs a, const u32 *__restrict__ keys, const PpSel *__restrict__ sel,
                                                               const int *__restrict__ ties, u64 *__restrict__ cand,
                                                               u32 *__restrict__ cand_n) {
    __shared__ int lds[4];
    __shared__ int wbase[PP_THREADS / 64];
    const int p = blockIdx.y, chw = problem_chw(a, p);
    const int i0 = blockIdx.x * PP_CHUNK;
    const PpSel s = sel[p];
    if (i0 >= chw) return;
    int base = 0;                                        // ties at T in the chunks before this one
    if (!s.all) {
        int v = 0;
        for (int c = threadIdx.x; c < (int)blockIdx.x; c += PP_THREADS) v += ties[(size_t)p * a.nchunks + c];
        block_exclusive_scan(v, lds, base);
    }
    const u32 *kp = keys + (size_t)p * a.chw_max;
    u64 *cp = cand + (size_t)p * a.K;
    for (int e = 0; e < PP_CHUNK; e += PP_THREADS) {
        const int i = i0 + e + threadIdx.x;
        const long long key = i < chw ? (long long)kp[i] : -2;
        const bool tie = !s.all && key == s.T;
        int nt;
        const int rank = base + block_exclusive_scan(tie ? 1 : 0, lds, nt);
        base += nt;
        const bool take = key > s.T || (tie && rank < s.r);
        int wn;
        const int wr = wave_rank(take, wn);
        if (lane_id() == 0 && wn) wbase[threadIdx.x >> 6] = (int)atomicAdd(cand_n + p, (u32)wn);
        __syncthreads();
        if (take) {
            const int slot = wbase[threadIdx.x >> 6] + wr;
            if (slot < a.K) cp[slot] = ((u64)(u32)key << 32) | (u64)(0xffffffffu - (u32)i);
        }
        __syncthreads();
    }
}

// sort (score desc, index asc), decode (centernet_utils.py:217-257), POST_CENTER_LIMIT_RANGE, compaction in score order
__global__ __launch_bounds__(PP_THREADS) void pp_finish_kernel(PpArgs a, const u64 *__restrict__ cand, const u32 *__restrict__ cand_n,
                                                               float *__restrict__ sbox, float *__restrict__ sscore,
                                                               int *__restrict__ scls, int *__restrict__ scount) {
    extern __shared__ u64 srt[];                         // [KP2]
    __shared__ int lds[4];
    const int p = blockIdx.x, N = a.KP2;
    const int n = min((int)cand_n[p], a.K);
    const u64 *cp = cand + (size_t)p * a.K;
    for (int i = threadIdx.x; i < N; i += PP_THREADS) srt[i] = i < n ? cp[i] : 0ull;     // (0 sorts behind every key)
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < N; i += PP_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const u64 x = srt[i], y = srt[ixj];
                    if (((i & k) == 0) ? (x < y) : (x > y)) {
                        srt[i] = y;
                        srt[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
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

// suppression mask of each problem over its first n = min(count, NMS_PRE_MAXSIZE) boxes (nms_mask_kernel of iou3d.hip with a
// device-side n and box rows of D floats)
template <bool NORMAL>
__global__ __launch_bounds__(64) void pp_nms_mask_kernel(PpArgs a, const float *__restrict__ sbox, const int *__restrict__ scount,
                                                         u64 *__restrict__ mask) {
    const int col = blockIdx.x, row = blockIdx.y, p = blockIdx.z;
    const int n = min(scount[p], a.pre);
    if (col < row || row * 64 >= n || col * 64 >= n) return;
    __shared__ float cb[64 * 7];
    const int lane = threadIdx.x, D = a.D;
    const float *boxes = sbox + (size_t)p * a.K * D;
    const int ncol = min(n - col * 64, 64), nrow = min(n - row * 64, 64);
    for (int e = lane; e < ncol * 7; e += 64) cb[e] = boxes[(size_t)(col * 64 + e / 7) * D + e % 7];
    __syncthreads();
    if (lane >= nrow) return;
    const int me = row * 64 + lane;
    float bx[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) bx[j] = boxes[(size_t)me * D + j];
    u64 t = 0;
    for (int i = (row == col) ? lane + 1 : 0; i < ncol; ++i) {
        const float v = NORMAL ? iou_normal_dev(bx, cb + i * 7) : iou_bev_dev(bx, cb + i * 7);
        if (v > a.nms_thresh) t |= 1ull << i;
    }
    mask[((size_t)p * a.K + me) * a.cbk + col] = t;
}

// greedy keep list per problem (nms_reduce_kernel of iou3d.hip, one wave per problem)
__global__ __launch_bounds__(64) void pp_nms_reduce_kernel(PpArgs a, const u64 *__restrict__ mask, const int *__restrict__ scount,
                                                           int *__restrict__ keep, int *__restrict__ nkeep) {
    __shared__ u64 remv[PCD_POSTPROC_MAX_K / 64];
    const int p = blockIdx.x, lane = threadIdx.x, cbk = a.cbk;
    const int n = min(scount[p], a.pre);
    const u64 *mp = mask + (size_t)p * a.K * cbk;
    int *kp = keep + (size_t)p * a.K;
    for (int w = lane; w < cbk; w += 64) remv[w] = 0;
    __syncthreads();
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        const int blk = i >> 6, bit = i & 63;
        const u64 word = remv[blk];
        if (!((word >> bit) & 1ull)) {
            if (lane == 0) kp[kept] = i;
            ++kept;
            const int wlim = (n + 63) >> 6;
            for (int w = blk + lane; w < wlim; w += 64) remv[w] |= mp[(size_t)i * cbk + w];
            __syncthreads();
        }
    }
    if (lane == 0) nkeep[p] = kept;
}

// per frame: the heads' kept boxes (first NMS_POST_MAXSIZE each) in head order, zeros behind
__global__ __launch_bounds__(PP_THREADS) void pp_output_kernel(PpArgs a, const float *__restrict__ sbox, const float *__restrict__ sscore,
                                                               const int *__restrict__ scls, const int *__restrict__ keep,
                                                               const int *__restrict__ nkeep, float *__restrict__ boxes,
                                                               float *__restrict__ scores, long long *__restrict__ labels,
                                                               int32_t *__restrict__ count) {
    const int b = blockIdx.x, D = a.D, M = a.NH * a.post;
    float *ob = boxes + (size_t)b * M * D;
    float *os = scores + (size_t)b * M;
    long long *ol = labels + (size_t)b * M;
    int off = 0;
    for (int h = 0; h < a.NH; ++h) {
        const int p = b * a.NH + h;
        const int k = min(nkeep[p], a.post);
        const int *kp = keep + (size_t)p * a.K;
        for (int j = threadIdx.x; j < k; j += PP_THREADS) {
            const int src = kp[j];
            const size_t q = (size_t)p * a.K + src;
            for (int d = 0; d < D; ++d) ob[(size_t)(off + j) * D + d] = sbox[q * D + d];
            os[off + j] = sscore[q];
            ol[off + j] = a.h[h].label[scls[q]];
        }
        off += k;
    }
    for (int j = off + threadIdx.x; j < M; j += PP_THREADS) {
        for (int d = 0; d < D; ++d) ob[(size_t)j * D + d] = 0.f;
        os[j] = 0.f;
        ol[j] = 0;
    }
    if (threadIdx.x == 0) count[b] = off;
}

struct PpLayout {
    size_t zero_bytes, total;
    size_t o_hist1, o_hist2, o_cand_n, o_keys, o_sel, o_ties, o_cand, o_sbox, o_sscore, o_scls, o_scount, o_mask, o_keep, o_nkeep;
};

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

PpLayout pp_layout(const PpArgs &a) {
    PpLayout l{};
    const size_t P = (size_t)a.B * a.NH, K = a.K;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += pcd_align_up(bytes, 256); return o; };
    l.o_hist1 = take(P * PP_BINS * 4);
    l.o_hist2 = take(P * PP_BINS * 4);
    l.o_cand_n = take(P * 4);
    l.zero_bytes = off;
    l.o_keys = take(P * (size_t)a.chw_max * 4);
    l.o_sel = take(P * sizeof(PpSel));
    l.o_ties = take(P * (size_t)a.nchunks * 4);
    l.o_cand = take(P * K * 8);
    l.o_sbox = take(P * K * a.D * 4);
    l.o_sscore = take(P * K * 4);
    l.o_scls = take(P * K * 4);
    l.o_scount = take(P * 4);
    l.o_mask = take(P * K * a.cbk * 8);
    l.o_keep = take(P * K * 4);
    l.o_nkeep = take(P * 4);
    l.total = off;
    return l;
}

}  // namespace

extern "C" size_t pcd_centerhead_postproc_workspace_bytes(const PcdPostprocHead *heads, const PcdPostprocConfig *cfg) {
    PpArgs a;
    if (pp_setup(heads, cfg, a) != PCD_OK) return 0;
    return pp_layout(a).total;
}

extern "C" int pcd_centerhead_postproc(const PcdPostprocHead *heads, const PcdPostprocConfig *cfg, float *boxes, float *scores,
                                       long long *labels, int32_t *count, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    PCD_ENTER();
    PpArgs a;
    const int rc = pp_setup(heads, cfg, a);
    if (rc != PCD_OK) return rc;
    if (!boxes || !scores || !labels || !count) return PCD_ERR_INVALID_ARG;
    const PpLayout l = pp_layout(a);
    if (!workspace || workspace_bytes < l.total || ((uintptr_t)workspace & 255)) return PCD_ERR_WORKSPACE;
    char *ws = (char *)workspace;
    u32 *hist1 = (u32 *)(ws + l.o_hist1), *hist2 = (u32 *)(ws + l.o_hist2), *cand_n = (u32 *)(ws + l.o_cand_n);
    u32 *keys = (u32 *)(ws + l.o_keys);
    PpSel *sel = (PpSel *)(ws + l.o_sel);
    int *ties = (int *)(ws + l.o_ties);
    u64 *cand = (u64 *)(ws + l.o_cand);
    float *sbox = (float *)(ws + l.o_sbox), *sscore = (float *)(ws + l.o_sscore);
    int *scls = (int *)(ws + l.o_scls), *scount = (int *)(ws + l.o_scount);
    u64 *mask = (u64 *)(ws + l.o_mask);
    int *keep = (int *)(ws + l.o_keep), *nkeep = (int *)(ws + l.o_nkeep);
    hipStream_t st = (hipStream_t)stream;
    const unsigned P = (unsigned)(a.B * a.NH);
    const dim3 stream_grid((unsigned)a.nchunks, P);
    pcd_fill(ws, 0, l.zero_bytes, st);
    pp_keys_kernel<<<stream_grid, PP_THREADS, 0, st>>>(a, keys, hist1);
    pp_find1_kernel<<<P, PP_THREADS, 0, st>>>(a, hist1, sel);
    pp_hist2_kernel<<<stream_grid, PP_THREADS, 0, st>>>(a, keys, sel, hist2);
    pp_find2_kernel<<<P, PP_THREADS, 0, st>>>(a, hist2, sel);
    pp_ties_kernel<<<stream_grid, PP_THREADS, 0, st>>>(a, keys, sel, ties);
    pp_gather_kernel<<<stream_grid, PP_THREADS, 0, st>>>(a, keys, sel, ties, cand, cand_n);
    pp_finish_kernel<<<P, PP_THREADS, (size_t)a.KP2 * sizeof(u64), st>>>(a, cand, cand_n, sbox, sscore, scls, scount);
    const dim3 tiles((unsigned)a.cbk, (unsigned)a.cbk, P);
    if (a.cbk > 0) {
        if (cfg->nms_normal)
            pp_nms_mask_kernel<true><<<tiles, 64, 0, st>>>(a, sbox, scount, mask);
        else
            pp_nms_mask_kernel<false><<<tiles, 64, 0, st>>>(a, sbox, scount, mask);
    }
    pp_nms_reduce_kernel<<<P, 64, 0, st>>>(a, mask, scount, keep, nkeep);
    pp_output_kernel<<<(unsigned)a.B, PP_THREADS, 0, st>>>(a, sbox, sscore, scls, keep, nkeep, boxes, scores, labels, count);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
