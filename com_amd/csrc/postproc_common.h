// The core of the static post-processing (postproc.hip: centre heads; anchor_postproc.hip: AnchorHeadSingle): the top-K
// selection with a total order, the LDS sort of the selected keys, the batched class-agnostic NMS and the per-frame output,
// for P independent "problems" in a fixed number of launches with grids from the shapes alone.  What a head brings is its
// ARGUMENT STRUCT `A` (passed by value to every kernel), the key producer among its members:
//     int K, KP2, pre, post, D, NH, chw_max, nchunks, cbk;  long long thr;  float nms_thresh;
//     __device__ int  count(int p)            elements of problem p (<= chw_max)
//     __device__ u32  key(int p, int i)       the 32-bit key of element i: orders like the score, larger first
//     __device__ int  out_label(int h, int c) the output label of what the finish kernel stored as class c of head h
// and its own finish kernel (sort -> decode -> sbox / sscore / scls / scount), built on sel_load_sort below.
//
// Order of the selection (total): key descending, equal keys by element index ascending; an element takes part iff
// (long long)key > thr.  (key << 32) | (0xffffffff - index) is one unique 64-bit key per element; the selection finds the
// K-th largest of them with two 16-bit histogram passes, counts the ties at the cut per chunk (chunks are index ranges) and
// gathers everything above the cut plus the first r ties by index.  Workgroups never hand data to each other inside a
// launch; the only atomics are integer adds (histograms, candidate slots), and the candidates are sorted by their unique
// keys afterwards, so slot order never shows.  Include inside the translation unit (everything is file-local).
#pragma once
#include "common.h"
#include "iou3d_geom.h"

namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_CHUNK = 2048;                 // elements per block of the streaming launches (8 per thread)
constexpr int PP_BINS = 65536;                 // 16-bit digits

// per-problem selection state (find launches -> later launches)
struct PpSel {
    int all;                                   // fewer than K pass: take every passing element
    int b1;                                    // high digit of the cut
    int above;                                 // keys above the cut's bin (pass 1), above T (pass 2)
    int r;                                     // ties at T still taken
    long long T;                               // take key > T (+ the first r with key == T)
    long long pad;
};

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

// keys[p][i] = a.key(p, i); hist1[p][key >> 16] counts the elements that take part
template <class A>
__global__ __launch_bounds__(PP_THREADS) void pp_keys_kernel(A a, u32 *__restrict__ keys, u32 *__restrict__ hist1) {
    const int p = blockIdx.y, chw = a.count(p);
    const int i0 = blockIdx.x * PP_CHUNK;
    if (i0 >= chw) return;
    u32 *kp = keys + (size_t)p * a.chw_max;
    u32 *hp = hist1 + (size_t)p * PP_BINS;
    for (int e = 0; e < PP_CHUNK; e += PP_THREADS) {
        const int i = i0 + e + threadIdx.x;
        const bool in = i < chw;
        u32 key = 0;
        if (in) {
            key = a.key(p, i);
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

__global__ __launch_bounds__(PP_THREADS) void pp_find1_kernel(int K, long long thr, const u32 *__restrict__ hist1,
                                                              PpSel *__restrict__ sel) {
    __shared__ int lds[8];
    const int p = blockIdx.x;
    const u32 *hp = hist1 + (size_t)p * PP_BINS;
    int sum = 0;
    for (int j = threadIdx.x; j < PP_BINS; j += PP_THREADS) sum += (int)hp[j];
    int total;
    block_exclusive_scan(sum, lds, total);
    if (total <= K) {                                    // every passing element is selected
        if (threadIdx.x == 0) {
            PpSel s = {};
            s.all = 1;
            s.T = thr;
            s.above = total;
            sel[p] = s;
        }
        return;
    }
    int bin, above;
    find_cut(hp, K, lds, bin, above);
    if (threadIdx.x == 0) {
        PpSel s = {};
        s.all = 0;
        s.b1 = bin;
        s.above = above;
        sel[p] = s;
    }
}

// low 16 bits of the passing keys inside the cut's bin
template <class A>
__global__ __launch_bounds__(PP_THREADS) void pp_hist2_kernel(A a, const u32 *__restrict__ keys, const PpSel *__restrict__ sel,
                                                              u32 *__restrict__ hist2) {
    const int p = blockIdx.y, chw = a.count(p);
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

__global__ __launch_bounds__(PP_THREADS) void pp_find2_kernel(int K, const u32 *__restrict__ hist2, PpSel *__restrict__ sel) {
    __shared__ int lds[8];
    const int p = blockIdx.x;
    const PpSel s = sel[p];
    if (s.all) return;
    int bin, above;
    find_cut(hist2 + (size_t)p * PP_BINS, K - s.above, lds, bin, above);
    if (threadIdx.x == 0) {
        PpSel o = s;
        o.T = ((long long)s.b1 << 16) | bin;
        o.above = s.above + above;                       // keys > T
        o.r = K - o.above;                               // >= 1 ties at T taken
        sel[p] = o;
    }
}

// elements with key == T per chunk
template <class A>
__global__ __launch_bounds__(PP_THREADS) void pp_ties_kernel(A a, const u32 *__restrict__ keys, const PpSel *__restrict__ sel,
                                                             int *__restrict__ ties) {
    __shared__ int lds[4];
    const int p = blockIdx.y, chw = a.count(p);
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
template <class A>
__global__ __launch_bounds__(PP_THREADS) void pp_gather_kernel(A a, const u32 *__restrict__ keys, const PpSel *__restrict__ sel,
                                                               const int *__restrict__ ties, u64 *__restrict__ cand,
                                                               u32 *__restrict__ cand_n) {
    __shared__ int lds[4];
    __shared__ int wbase[PP_THREADS / 64];
    const int p = blockIdx.y, chw = a.count(p);
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

// The first part of a finish kernel: the n <= K candidates of problem p into srt[KP2] (LDS), sorted by (key desc, index
// asc); returns n.  Every thread of the block calls it; ends with a barrier.
__device__ __forceinline__ int sel_load_sort(const u64 *__restrict__ cand, const u32 *__restrict__ cand_n, int p, int K, int KP2,
                                             u64 *srt) {
    const int N = KP2;
    const int n = min((int)cand_n[p], K);
    const u64 *cp = cand + (size_t)p * K;
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
    return n;
}

// suppression mask of each problem over its first n = min(count, NMS_PRE_MAXSIZE) boxes (nms_mask_kernel of iou3d.hip with a
// device-side n and box rows of D floats)
template <bool NORMAL>
__global__ __launch_bounds__(64) void pp_nms_mask_kernel(int K, int D, int pre, int cbk, float nms_thresh,
                                                         const float *__restrict__ sbox, const int *__restrict__ scount,
                                                         u64 *__restrict__ mask) {
    const int col = blockIdx.x, row = blockIdx.y, p = blockIdx.z;
    const int n = min(scount[p], pre);
    if (col < row || row * 64 >= n || col * 64 >= n) return;
    __shared__ float cb[64 * 7];
    const int lane = threadIdx.x;
    const float *boxes = sbox + (size_t)p * K * D;
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
        if (v > nms_thresh) t |= 1ull << i;
    }
    mask[((size_t)p * K + me) * cbk + col] = t;
}

// greedy keep list per problem (nms_reduce_kernel of iou3d.hip, one wave per problem)
__global__ __launch_bounds__(64) void pp_nms_reduce_kernel(int K, int pre, int cbk, const u64 *__restrict__ mask,
                                                           const int *__restrict__ scount, int *__restrict__ keep,
                                                           int *__restrict__ nkeep) {
    __shared__ u64 remv[PCD_POSTPROC_MAX_K / 64];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int n = min(scount[p], pre);
    const u64 *mp = mask + (size_t)p * K * cbk;
    int *kp = keep + (size_t)p * K;
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
template <class A>
__global__ __launch_bounds__(PP_THREADS) void pp_output_kernel(A a, const float *__restrict__ sbox, const float *__restrict__ sscore,
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
            ol[off + j] = a.out_label(h, scls[q]);
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

// ---- workspace and the launches every head shares -------------------------------------------------------------------------
struct PpLayout {
    size_t zero_bytes, total;
    size_t o_hist1, o_hist2, o_cand_n, o_keys, o_sel, o_ties, o_cand, o_sbox, o_sscore, o_scls, o_scount, o_mask, o_keep, o_nkeep;
};

PpLayout pp_layout(size_t P, size_t K, int D, int chw_max, int nchunks, int cbk) {
    PpLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += pcd_align_up(bytes, 256); return o; };
    l.o_hist1 = take(P * PP_BINS * 4);
    l.o_hist2 = take(P * PP_BINS * 4);
    l.o_cand_n = take(P * 4);
    l.zero_bytes = off;
    l.o_keys = take(P * (size_t)chw_max * 4);
    l.o_sel = take(P * sizeof(PpSel));
    l.o_ties = take(P * (size_t)nchunks * 4);
    l.o_cand = take(P * K * 8);
    l.o_sbox = take(P * K * D * 4);
    l.o_sscore = take(P * K * 4);
    l.o_scls = take(P * K * 4);
    l.o_scount = take(P * 4);
    l.o_mask = take(P * K * cbk * 8);
    l.o_keep = take(P * K * 4);
    l.o_nkeep = take(P * 4);
    l.total = off;
    return l;
}

struct PpBuffers {
    u32 *hist1, *hist2, *cand_n, *keys;
    PpSel *sel;
    int *ties;
    u64 *cand;
    float *sbox, *sscore;
    int *scls, *scount;
    u64 *mask;
    int *keep, *nkeep;
};

PpBuffers pp_buffers(void *workspace, const PpLayout &l) {
    char *ws = (char *)workspace;
    PpBuffers w;
    w.hist1 = (u32 *)(ws + l.o_hist1);
    w.hist2 = (u32 *)(ws + l.o_hist2);
    w.cand_n = (u32 *)(ws + l.o_cand_n);
    w.keys = (u32 *)(ws + l.o_keys);
    w.sel = (PpSel *)(ws + l.o_sel);
    w.ties = (int *)(ws + l.o_ties);
    w.cand = (u64 *)(ws + l.o_cand);
    w.sbox = (float *)(ws + l.o_sbox);
    w.sscore = (float *)(ws + l.o_sscore);
    w.scls = (int *)(ws + l.o_scls);
    w.scount = (int *)(ws + l.o_scount);
    w.mask = (u64 *)(ws + l.o_mask);
    w.keep = (int *)(ws + l.o_keep);
    w.nkeep = (int *)(ws + l.o_nkeep);
    return w;
}

// fill, keys, find 1, hist 2, find 2, ties, gather: the candidates of all P problems (7 launches)
template <class A>
void pp_launch_select(const A &a, unsigned P, void *workspace, const PpLayout &l, const PpBuffers &w, hipStream_t st) {
    const dim3 stream_grid((unsigned)a.nchunks, P);
    pcd_fill(workspace, 0, l.zero_bytes, st);
    pp_keys_kernel<<<stream_grid, PP_THREADS, 0, st>>>(a, w.keys, w.hist1);
    pp_find1_kernel<<<P, PP_THREADS, 0, st>>>(a.K, a.thr, w.hist1, w.sel);
    pp_hist2_kernel<<<stream_grid, PP_THREADS, 0, st>>>(a, w.keys, w.sel, w.hist2);
    pp_find2_kernel<<<P, PP_THREADS, 0, st>>>(a.K, w.hist2, w.sel);
    pp_ties_kernel<<<stream_grid, PP_THREADS, 0, st>>>(a, w.keys, w.sel, w.ties);
    pp_gather_kernel<<<stream_grid, PP_THREADS, 0, st>>>(a, w.keys, w.sel, w.ties, w.cand, w.cand_n);
}

// nms mask, nms reduce, output: from the finish kernel's sorted boxes to the padded outputs (3 launches)
template <class A>
void pp_launch_nms_output(const A &a, unsigned P, unsigned frames, bool normal, const PpBuffers &w, float *boxes, float *scores,
                          long long *labels, int32_t *count, hipStream_t st) {
    const dim3 tiles((unsigned)a.cbk, (unsigned)a.cbk, P);
    if (a.cbk > 0) {
        if (normal)
            pp_nms_mask_kernel<true><<<tiles, 64, 0, st>>>(a.K, a.D, a.pre, a.cbk, a.nms_thresh, w.sbox, w.scount, w.mask);
        else
            pp_nms_mask_kernel<false><<<tiles, 64, 0, st>>>(a.K, a.D, a.pre, a.cbk, a.nms_thresh, w.sbox, w.scount, w.mask);
    }
    pp_nms_reduce_kernel<<<P, 64, 0, st>>>(a.K, a.pre, a.cbk, w.mask, w.scount, w.keep, w.nkeep);
    pp_output_kernel<<<frames, PP_THREADS, 0, st>>>(a, w.sbox, w.sscore, w.scls, w.keep, w.nkeep, boxes, scores, labels, count);
}

}  // namespace
